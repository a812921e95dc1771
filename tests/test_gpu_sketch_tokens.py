"""``--sketch_attn tokens`` on the device: the whole model (``build_model``, --backbone features) with every video token attending to
the sketch's tokens, against the fp64 restatement tests/sketch_tokens_ref.py.  hidden_dim 64 / nheads 2 (d_h = 32: in bf16 / fp16 the
video -> sketch attention runs on the few-keys kernels, in fp32 on the generic ones: the tight bar that catches wiring errors), 2 layers,
8 queries, T = 4 frames of P = 6 tokens, input widths 48, Ls = 5 sketch tokens, the last two of batch row 1 padding.

  * outputs of every layer, the loss and every parameter gradient against the reference, on the bars gpu_checks.check_head_case holds
    gate-mode heads to: absolute 1e-3 fp32 / 1e-2 bf16 / 3e-3 fp16 on logits and boxes, grad_bars' element and norm-wise bars, fp16
    under its loss scale; the reference's criterion runs at the device's own assignment (as there);
  * padding works: garbage (NaN, 1e30) in the padded tokens' features leaves every output bit-identical;
  * the model sees the sketch: permuting the valid sketch tokens moves the logits by more than the bar with --use_sketch_pos (the
    reference: 0.12 at layer 0, 0.044 at the last) and leaves them within it without positions;
  * sketch_video_cross_attn.out_proj trains; the few-keys ops run once per layer and direction in bf16 / fp16 and never in fp32;
  * gate mode is untouched: a default-built model at Ls = 1 never calls the new ops.
"""
from __future__ import annotations

import functools

import pytest
import torch

from tests import sketch_tokens_ref as R

pytestmark = pytest.mark.gpu

DEV = 'cuda'
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
NAMES = {torch.float32: 'fp32', torch.bfloat16: 'bf16', torch.float16: 'fp16'}
TOL = {torch.float32: 1e-3, torch.bfloat16: 1e-2, torch.float16: 3e-3}     # gpu_checks.check_head_case


def build(dtype, **over):
    from svol_amd import synthetic as syn
    from svol_amd.modeling.loss import build_loss
    from svol_amd.modeling.model import build_model
    args = R.case_args(**over)
    args.compute_dtype = NAMES[dtype]
    model = build_model(args)
    model.head.load_state_dict(syn.synth_state_dict(args, seed=1), strict=True)
    return args, model.to(DEV).eval(), build_loss(args).to(DEV).eval()


def forward(model, inp):
    return model(inp['src_sketch'].to(DEV), inp['src_video'].to(DEV), inp['src_sketch_mask'].to(DEV), inp['src_video_mask'].to(DEV))


def stacked(out):
    """(logits, boxes) of every layer, aux first -> [nl, B, N, .] on the CPU"""
    lay = list(out.get('aux_outputs', [])) + [out]
    return (torch.stack([a['pred_logits'].detach() for a in lay]).double().cpu(),
            torch.stack([a['pred_boxes'].detach() for a in lay]).double().cpu())


class Counter:
    """counts the calls of the few-keys ops"""

    def __init__(self, monkeypatch):
        from svol_amd import ops
        self.n = {'fwd': 0, 'bwd': 0}
        for key, name in (('fwd', 'attn_fewkeys_fwd'), ('bwd', 'attn_fewkeys_bwd')):
            monkeypatch.setattr(ops, name, self._wrap(getattr(ops, name), key))

    def _wrap(self, fn, key):
        def f(*a, **k):
            self.n[key] += 1
            return fn(*a, **k)
        return f


@functools.lru_cache(maxsize=None)
def device_run(dtype):
    """forward, criterion and backward on the device, once per type -> dict (shared, never modified)"""
    from svol_amd import synthetic as syn
    from tests import gpu_checks as G
    args, model, crit = build(dtype)
    inp = R.case_inputs(args)
    tg = syn.synth_targets(R.B, R.T, seed=1)
    out = forward(model, inp)
    ld = crit(out, tg)
    wd = crit.weight_dict
    tot = sum(ld[k] * wd[k] for k in ld.keys() if k in wd)
    scale = G.FP16_LOSS_SCALE if dtype == torch.float16 else 1.0
    (tot * scale).backward()
    if scale != 1.0:
        with torch.no_grad():
            for p_ in model.parameters():
                if p_.grad is not None:
                    p_.grad.mul_(1.0 / scale)
    torch.cuda.synchronize()
    idx = [[(p.cpu().numpy(), t.cpu().numpy()) for p, t in lay] for lay in crit.last_indices()]     # [aux0.., last]
    return dict(args=args, model=model, inp=inp, tg=tg, out=out, tot=float(tot), idx=idx)


@functools.lru_cache(maxsize=None)
def reference_at(dtype):
    """the fp64 reference at the device run's own assignment (the matcher is @no_grad: the loss is a function of the outputs and it)"""
    d = device_run(dtype)
    return R.reference_run(d['args'], d['inp'], d['tg'], indices=d['idx'][-1:] + d['idx'][:-1])


@pytest.mark.parametrize('dtype', DTYPES, ids=NAMES.values())
def test_outputs_loss_and_gradients_against_fp64(dtype):
    from tests import gpu_checks as G
    d = device_run(dtype)
    r_out, _, r_tot, r_grads, _ = reference_at(dtype)
    tol = TOL[dtype]
    res = {}
    for tag, got, ref in zip(('logits', 'boxes'), stacked(d['out']), stacked(r_out)):
        assert bool(torch.isfinite(got).all()), tag
        res[f'{tag}_abs (all layers)'] = (float((got - ref).abs().max()), tol)
    res['loss_total_vs_reference_at_device_assignment'] = (abs(d['tot'] - float(r_tot)), tol * max(1.0, abs(float(r_tot))))
    res.update(G.compare_param_grads(f'sketch_tokens/{NAMES[dtype]}', d['model'].head, r_grads, dtype, G.grad_bars(dtype, d['args'].hidden_dim)))
    bad = []
    for k, (val, bar) in res.items():
        print(f'{NAMES[dtype]} {k}: {val:.3e} (<= {bar:.3e})')
        if not val <= bar:
            bad.append(f'{k}: {val:.3e} vs {bar:.3e}')
    assert not bad, '; '.join(bad)
    for li in range(d['args'].num_layers):
        g = dict(d['model'].head.named_parameters())[f'transformer.layers.{li}.sketch_video_cross_attn.out_proj.weight'].grad
        assert g is not None and float(g.abs().max()) > 0.0, li


@pytest.mark.parametrize('dtype', DTYPES, ids=NAMES.values())
def test_padded_sketch_tokens_reach_nothing(dtype):
    d = device_run(dtype)
    base = stacked(d['out'])
    junk = dict(d['inp'], src_sketch=d['inp']['src_sketch'].clone())
    junk['src_sketch'][R.PAD_ROW, R.LS - R.PAD_TOKENS] = float('nan')
    junk['src_sketch'][R.PAD_ROW, R.LS - 1] = 1e30
    with torch.no_grad():
        got = stacked(forward(d['model'], junk))
    for a, b in zip(got, base):
        assert torch.equal(a, b)


@pytest.mark.parametrize('dtype', DTYPES, ids=NAMES.values())
def test_the_model_sees_the_sketch_tokens_order_only_through_positions(dtype):
    d = device_run(dtype)
    perm = dict(d['inp'], src_sketch=d['inp']['src_sketch'].clone())
    perm['src_sketch'][:, :3] = d['inp']['src_sketch'][:, [2, 0, 1]]      # the valid tokens of both rows
    with torch.no_grad():
        moved = float((stacked(forward(d['model'], perm))[0] - stacked(d['out'])[0]).abs().max())
        _, plain, _ = build(dtype, use_sketch_pos=False)
        still = float((stacked(forward(plain, perm))[0] - stacked(forward(plain, d['inp']))[0]).abs().max())
    print(f'{NAMES[dtype]}: permuted sketch tokens move the logits by {moved:.3e} with positions, {still:.3e} without (bar {TOL[dtype]:.0e})')
    assert moved > TOL[dtype] and still <= TOL[dtype]


@pytest.mark.parametrize('dtype', DTYPES, ids=NAMES.values())
def test_fewkeys_ops_run_where_the_shape_qualifies(dtype, monkeypatch):
    from svol_amd import synthetic as syn
    c = Counter(monkeypatch)
    args, model, crit = build(dtype)
    out = forward(model, R.case_inputs(args))
    ld = crit(out, syn.synth_targets(R.B, R.T, seed=1))
    sum(ld[k] * crit.weight_dict[k] for k in ld.keys() if k in crit.weight_dict).backward()
    torch.cuda.synchronize()
    want = 0 if dtype == torch.float32 else args.num_layers
    assert c.n == {'fwd': want, 'bwd': want}


def test_gate_mode_never_calls_the_new_ops(monkeypatch):
    from svol_amd import synthetic as syn
    c = Counter(monkeypatch)
    args, model, crit = build(torch.bfloat16, sketch_attn='gate')
    assert all(layer.sketch_attn == 'gate' for layer in model.head.transformer.layers)
    inp = R.case_inputs(args)
    inp = dict(inp, src_sketch=inp['src_sketch'][:, :1].contiguous(), src_sketch_mask=torch.ones((R.B, 1)))
    out = forward(model, inp)
    again = forward(model, inp)
    ld = crit(out, syn.synth_targets(R.B, R.T, seed=1))
    sum(ld[k] * crit.weight_dict[k] for k in ld.keys() if k in crit.weight_dict).backward()
    torch.cuda.synchronize()
    assert c.n == {'fwd': 0, 'bwd': 0}
    for a, b in zip(stacked(out), stacked(again)):
        assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    g = dict(model.head.named_parameters())['transformer.layers.0.sketch_video_cross_attn.out_proj.weight'].grad
    assert g is None or float(g.abs().max()) == 0.0
