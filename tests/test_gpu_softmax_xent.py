"""svol_softmax_xent (csrc/sketch_cls.hip) against F.cross_entropy in fp64: the mean loss (<= 1e-5 relative), dlogits = (softmax -
onehot) / n (<= gpu_checks.TOL[fp32] of its largest entry, every row summing to <= 1e-6), the top-1 hit count (no ties in the inputs),
bit-identical repeats, the refusal of C = 1025, and out-of-range targets (C and -1, on middle rows only, so that even a kernel that
used them as an index would stay inside the allocation): the loss is NaN, that row of dlogits is NaN, the other rows are finite.

The device's worst figures over the cases: loss 1.4e-7 relative (n = 5, C = 65, peaked), dlogits 1.7e-7 of its largest entry (n = 257,
C = 21), row sums 3.4e-8 (n = 3, C = 19)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CASES = [(1, 1), (1, 2), (3, 19), (32, 24), (5, 64), (5, 65), (7, 1024), (257, 21)]
FAMILIES = ('randn3', 'peaked')


def _inputs(n, C, family, ld=None):
    """-> (logits [n, C] fp32 as a view of [n, ld], targets [n]); no two entries of a row are equal"""
    g = torch.Generator().manual_seed(1000 * n + C)
    buf = torch.full((n, ld or C), 123.0)
    x = buf[:, :C]
    x.copy_(torch.randn(n, C, generator=g) * 3)
    t = torch.randint(0, C, (n,), generator=g)
    if family == 'peaked':
        hot = torch.randint(0, C, (n,), generator=g)
        sign = torch.where(torch.arange(n) % 2 == 0, 1e4, -1e4)
        x[torch.arange(n), hot] += sign
    for r in range(n):
        assert x[r].unique().numel() == C
    return x, t


def _check(x, t):
    from svol_amd import ops
    from tests import gpu_checks as G
    n, C = x.shape
    xd = (x if x.is_contiguous() else x._base).to(DEV)[:, :C]      # (the strided case keeps its leading dimension on the device)
    loss, dl, correct = ops.softmax_xent(xd, t.to(DEV))
    loss2, dl2, correct2 = ops.softmax_xent(xd, t.to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(loss, loss2) and torch.equal(dl, dl2) and torch.equal(correct, correct2)
    xr = x.double().clone().requires_grad_(True)
    ref = F.cross_entropy(xr, t)
    ref.backward()
    ref = ref.detach()
    e_loss = abs(float(loss) - float(ref)) / max(abs(float(ref)), 1e-300)
    e_dl = float((dl.cpu().double() - xr.grad).abs().max() / xr.grad.abs().max().clamp_min(1e-300))
    rowsum = float(dl.cpu().double().sum(1).abs().max())
    print(f'n={n} C={C}: loss {float(loss):.6e} (ref {float(ref):.6e}, rel {e_loss:.2e})  dlogits {e_dl:.2e}  rowsum {rowsum:.2e}')
    assert e_loss <= 1e-5 or abs(float(loss) - float(ref)) == 0.0
    assert e_dl <= G.TOL[torch.float32] or float(xr.grad.abs().max()) == 0.0
    assert rowsum <= 1e-6
    assert int(correct) == int((x.argmax(1) == t).sum())
    assert bool(torch.isfinite(dl).all())


@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('n,C', CASES)
def test_against_fp64_cross_entropy(n, C, family):
    _check(*_inputs(n, C, family))


@pytest.mark.parametrize('family', FAMILIES)
def test_strided_logits(family):
    x, t = _inputs(6, 21, family, ld=40)
    assert not x.is_contiguous()
    _check(x, t)


def test_more_than_1024_classes_is_refused():
    from svol_amd import _lib, ops
    x = torch.zeros((2, 1025), device=DEV)
    with pytest.raises(_lib.SvolHipError, match='code -2'):
        ops.softmax_xent(x, torch.zeros(2, dtype=torch.int64, device=DEV))


@pytest.mark.parametrize('bad', [19, -1])
def test_out_of_range_target_gives_nan_and_reads_nothing(bad):
    from svol_amd import ops
    x, t = _inputs(5, 19, 'randn3')
    t[2] = bad
    loss, dl, _ = ops.softmax_xent(x.to(DEV), t.to(DEV))
    torch.cuda.synchronize()
    assert bool(torch.isnan(loss).all())
    assert bool(torch.isnan(dl[2]).all())
    keep = [0, 1, 3, 4]
    assert bool(torch.isfinite(dl[keep]).all())
    ref = torch.softmax(x.double(), 1)
    ref[torch.arange(5), t.clamp(0, 18)] -= 1
    assert float((dl[keep].cpu().double() - ref[keep] / 5).abs().max()) <= 2e-5
