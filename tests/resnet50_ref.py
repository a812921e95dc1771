"""fp64 restatement of the bottleneck ResNet extractor in plain torch.nn, with torchvision's key layout: the children of
``nn.Sequential(*list(torchvision.models.resnet50().children())[:-2])`` — ``0`` conv1, ``1`` bn1, ``4`` ... layer1 ..., blocks with
conv1/bn1 (1x1), conv2/bn2 (3x3, carries the stride), conv3/bn3 (1x1 to 4 * planes), downsample.{0,1} — so that its state dict loads
into svol_amd.modeling.resnet.ResNetExtractor(block='bottleneck') with strict=True.  Eval mode (running statistics), train mode (batch
statistics, running statistics updated as nn.BatchNorm2d does) and the optional global average pool.  Pinned to
transformers.ResNetModel(layer_type='bottleneck') by tests/test_resnet50_ref.py; the GPU tests compare the HIP extractors with it.
No GPU import.
"""
import torch
import torch.nn.functional as F
from torch import nn


class RefBottleneck(nn.Module):
    def __init__(self, inplanes, planes, stride):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, 1, 0, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, 4 * planes, 1, 1, 0, bias=False)
        self.bn3 = nn.BatchNorm2d(4 * planes)
        self.downsample = None
        if stride != 1 or inplanes != 4 * planes:
            self.downsample = nn.Sequential(nn.Conv2d(inplanes, 4 * planes, 1, stride, bias=False), nn.BatchNorm2d(4 * planes))

    def forward(self, x):
        t = F.relu(self.bn1(self.conv1(x)))
        t = F.relu(self.bn2(self.conv2(t)))
        t = self.bn3(self.conv3(t))
        return F.relu(t + (x if self.downsample is None else self.downsample(x)))


class RefBottleneckNet(nn.Module):
    """pixels [n,3,H,W] -> feature map [n, 4 * planes[-1], h, w], or [n, C] with avgpool"""

    def __init__(self, depths=(3, 4, 6, 3), planes=(64, 128, 256, 512), stem=64, avgpool=False):
        super().__init__()
        self.add_module('0', nn.Conv2d(3, stem, 7, 2, 3, bias=False))
        self.add_module('1', nn.BatchNorm2d(stem))
        inplanes = stem
        for li, (n, p) in enumerate(zip(depths, planes)):
            blocks = []
            for bi in range(n):
                blocks.append(RefBottleneck(inplanes, p, (1 if li == 0 else 2) if bi == 0 else 1))
                inplanes = 4 * p
            self.add_module(str(4 + li), nn.Sequential(*blocks))
        self.n_layers = len(depths)
        self.out_channels = inplanes
        self.avgpool = avgpool
        self.double()

    def forward(self, x):
        h = F.relu(getattr(self, '1')(getattr(self, '0')(x.double())))
        h = F.max_pool2d(h, 3, 2, 1)
        for li in range(self.n_layers):
            h = getattr(self, str(4 + li))(h)
        return F.adaptive_avg_pool2d(h, 1).flatten(1) if self.avgpool else h


def tokens(fmap):
    """[n, C, h, w] -> [n, h*w, C], row-major over (h, w): the extractor's token order"""
    return fmap.flatten(2).transpose(1, 2)


def synth_state_dict(net, seed):
    """deterministic weights that keep activations O(1) through the stack: He-scaled convolutions, BatchNorm weight 1 +- 0.1 (0.5 +- 0.05
    on a block's last BatchNorm: the identity add would otherwise double the scale per block), bias / running mean +- 0.1, running
    variance 1 +- 0.2"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, v in net.state_dict().items():
        if k.endswith('num_batches_tracked'):
            sd[k] = torch.zeros_like(v)
        elif v.dim() == 4:
            sd[k] = torch.randn(v.shape, generator=g) * (2.0 / (v.shape[1] * v.shape[2] * v.shape[3])) ** 0.5
        elif k.endswith('running_var'):
            sd[k] = 1.0 + 0.4 * (torch.rand(v.shape, generator=g) - 0.5)
        elif k.endswith('weight'):
            sd[k] = (0.5 if '.bn3.' in k else 1.0) * (1.0 + 0.2 * (torch.rand(v.shape, generator=g) - 0.5))
        else:
            sd[k] = 0.2 * (torch.rand(v.shape, generator=g) - 0.5)
    return sd


def synth_pixels(n, size, seed):
    return torch.randn((n, 3, size, size), generator=torch.Generator().manual_seed(seed))


def build(depths, planes, stem, seed, avgpool=False):
    net = RefBottleneckNet(depths, planes, stem, avgpool)
    sd = synth_state_dict(net, seed)
    net.load_state_dict(sd)
    return net, sd


# ---- the same network with the HIP path's 16-bit roundings (torch, any device): what the GPU tests' bars are derived from -------
class _Round(torch.autograd.Function):
    """x -> dt(x) in the forward AND the backward: where the HIP path keeps an activation / its gradient in a 16-bit type"""

    @staticmethod
    def forward(ctx, x, dt):
        ctx.dt = dt
        return x.to(dt).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g.to(ctx.dt).to(g.dtype), None


def _block_units(sd, depths):
    """(prefix, stride, has_downsample) of every block in order"""
    for li, nb in enumerate(depths):
        for bi in range(nb):
            p = f'{4 + li}.{bi}'
            yield p, ((1 if li == 0 else 2) if bi == 0 else 1), (p + '.downsample.0.weight') in sd


def emulate_frozen(sd, depths, x, dt):
    """eval mode in fp64 with roundings to `dt` where the product rounds: the BatchNorm-folded weights (folded in fp32), the pixels,
    every unit's output -> feature map [n, C, h, w] fp64.  (fp64 accumulation: the figure is the error of the ROUNDINGS alone)"""
    r = lambda t: t.to(dt).double()

    def unit(h, conv, bn, stride, pad, idt=None, relu=True):
        scale = sd[bn + '.weight'].float() / torch.sqrt(sd[bn + '.running_var'].float() + 1e-5)
        shift = sd[bn + '.bias'].float() - sd[bn + '.running_mean'].float() * scale
        z = F.conv2d(h, r(sd[conv + '.weight'].float() * scale[:, None, None, None]), shift.double(), stride, pad)
        if idt is not None:
            z = z + idt
        return r(torch.relu(z) if relu else z)
    h = unit(r(x.float()), '0', '1', 2, 3)
    h = F.max_pool2d(h, 3, 2, 1)
    for p, stride, down in _block_units(sd, depths):
        t = unit(h, p + '.conv1', p + '.bn1', 1, 0)
        t = unit(t, p + '.conv2', p + '.bn2', stride, 1)
        idt = unit(h, p + '.downsample.0', p + '.downsample.1', stride, 0, relu=False) if down else h
        h = unit(t, p + '.conv3', p + '.bn3', 1, 0, idt=idt)
    return h


def emulate_train(sd, depths, x, dt, probe_fmap=None, avg=False, device='cpu', ftype=torch.float64, loss_scale=1.0):
    """train mode (batch statistics) with the HIP path's roundings: conv weights (forward only), conv output, unit output, and the
    gradients of these two.  -> (features, {key: gradient} or None without a probe, {running statistic: value})"""
    r = lambda t: _Round.apply(t, dt)
    P = {k: (v.detach().to(device).to(ftype).requires_grad_('running' not in k) if v.is_floating_point() else v) for k, v in sd.items()}
    w = lambda k: P[k] + (P[k].detach().to(dt).to(ftype) - P[k].detach())
    stats = {}

    def bn(z, p):
        rm, rv = P[p + '.running_mean'].clone(), P[p + '.running_var'].clone()
        y = F.batch_norm(z, rm, rv, P[p + '.weight'], P[p + '.bias'], True, 0.1, 1e-5)
        stats[p + '.running_mean'], stats[p + '.running_var'] = rm, rv
        return y
    h = r(F.relu(bn(r(F.conv2d(r(x.to(device).to(ftype)), w('0.weight'), None, 2, 3)), '1')))
    h = F.max_pool2d(h, 3, 2, 1)
    for p, stride, down in _block_units(sd, depths):
        t = r(F.relu(bn(r(F.conv2d(h, w(p + '.conv1.weight'), None, 1, 0)), p + '.bn1')))
        t = r(F.relu(bn(r(F.conv2d(t, w(p + '.conv2.weight'), None, stride, 1)), p + '.bn2')))
        idt = r(bn(r(F.conv2d(h, w(p + '.downsample.0.weight'), None, stride, 0)), p + '.downsample.1')) if down else h
        h = r(F.relu(bn(r(F.conv2d(t, w(p + '.conv3.weight'), None, 1, 0)), p + '.bn3') + idt))
    f = F.adaptive_avg_pool2d(h, 1) if avg else h
    grads = None
    if probe_fmap is not None:
        (f * (probe_fmap.to(device).to(ftype) * loss_scale)).sum().backward()
        grads = {k: v.grad / loss_scale for k, v in P.items() if torch.is_tensor(v) and v.requires_grad}
    return f.detach(), grads, stats


def train_reference(net, x, probe_fmap=None):
    """the fp64 restatement in train mode on a COPY of net: (features, {key: gradient} or None, {running statistic: value})"""
    import copy
    m = copy.deepcopy(net).train()
    f = m(x)
    grads = None
    if probe_fmap is not None:
        (f * probe_fmap.double().view(f.shape)).sum().backward()
        grads = {k: p.grad for k, p in m.named_parameters()}
    return f.detach(), grads, {k: b.detach() for k, b in m.named_buffers() if 'running' in k}
