"""--nheads above eight through the product modules: the SVANet head against reference-generated fixtures with 9, 12, 16 and 32 heads
(tests/golden/make_golden_heads.py; the CPU oracle is held to the same fixtures in tests/test_oracle_golden_heads.py), and one training
step through build_model at hidden_dim 512 / nheads 16 (heads of 32: the tuned 16-bit attention kernels) and 256 / 16 (heads of 16).
Every sketch -> video gate here runs in more than one group of eight heads (csrc/gate.hip); the bars are those of the checks called,
none new.  The kernels themselves are looked at in tests/test_gpu_gate_heads.py: a model's outputs are nearly blind to the gate."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

_DT = {'fp32': torch.float32, 'bf16': torch.bfloat16, 'fp16': torch.float16}


def _hold(res):
    for k, (e, t) in res.items():
        print(f'{k}: err={e:.3e} tol={t:.1e}{"" if e <= t else "   <-- FAILS"}')
    bad = {k: v for k, v in res.items() if not (v[0] <= v[1])}
    assert not bad, '\n'.join(f'{k}: err={e:.3e} tol={t:.1e}' for k, (e, t) in bad.items())


@pytest.mark.parametrize('dtype', ['fp32', 'bf16', 'fp16'])
@pytest.mark.parametrize('name', ['h9_video', 'h12_frame', 'h16_video', 'h32_frame'])
def test_head_golden(name, dtype):
    from tests import gpu_checks as G
    _hold(G.check_head_case(name, _DT[dtype]))


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_head_golden_gradient_sinks(dtype):
    from tests import gpu_checks as G
    _hold(G.check_head_case('h16_video', _DT[dtype], sinks=True))


def _svanet_step(hidden_dim, nheads, per_op):
    """one SVANet training step through build_model, bf16, gradient sinks + FlatAdamW"""
    from svol_amd import blocks, parallel
    from svol_amd import synthetic as syn
    from svol_amd.modeling.loss import build_loss
    from svol_amd.modeling.model import build_model
    B, T, P, N = 2, 4, 49, 16
    args = syn.head_args(hidden_dim=hidden_dim, nheads=nheads, num_layers=2, num_queries=N, num_queries_per_frame=4, num_frames=T,
                         input_vid_dim=64, input_skch_dim=64, input_dropout=0.0, matcher='video_matcher', backbone='features')
    args.compute_dtype = 'bf16'
    sd = syn.synth_state_dict(args, seed=3)
    inp = syn.synth_inputs(args, B, T, P, seed=3, pad_frames=1)
    tg = syn.synth_targets(B, T, seed=3)
    default = blocks.ENABLED
    try:
        blocks.ENABLED = default and not per_op
        model = build_model(args)
        model.load_state_dict({'head.' + k: v for k, v in sd.items()}, strict=True)
        model = model.cuda().train()
        crit = build_loss(args).cuda().train()
        params = [p for p in model.parameters() if p.requires_grad]
        skip = parallel.unused_parameters(model)
        red = parallel.BucketedGradAllReduce(params, skip=skip)
        opt = parallel.FlatAdamW(red, lr=1e-3, weight_decay=1e-4)
        red.zero_grad()
        frame_mask = inp['src_video_mask'].view(B, T, P)[:, :, 0].contiguous()
        out = model(src_sketch=inp['src_sketch'].cuda(), src_video=inp['src_video'].view(B, T, P, -1).cuda(),
                    src_sketch_mask=inp['src_sketch_mask'].cuda(), src_video_mask=frame_mask.cuda())
        ld = crit(out, tg)
        loss = crit.weighted_total()
        loss.backward()
        red.finish()
        torch.cuda.synchronize()
        skipped = {id(p) for p in skip}
        grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.requires_grad and id(p) not in skipped}
        before = {n: p.detach().clone() for n, p in model.named_parameters()}
        opt.step()
        torch.cuda.synchronize()
        moved = sum(int(not torch.equal(before[n], p.detach())) for n, p in model.named_parameters())
    finally:
        blocks.ENABLED = default
    lays = list(out.get('aux_outputs', [])) + [out]
    return dict(outs=[(o['pred_logits'].detach(), o['pred_boxes'].detach()) for o in lays], losses={k: float(v) for k, v in ld.items()},
                total=float(loss), grads=grads, moved=moved)


@pytest.mark.parametrize('hidden_dim', [512, 256])
def test_svanet_step_at_nheads_16_through_build_model(hidden_dim):
    """nheads 16, two layers, T = 4, P = 49, N = 16, bf16: forward, criterion, backward, one FlatAdamW step -- through the block programs
    and through the per-op path.  The two run the same kernels in the same order: forward outputs bit-identical (the bar of
    tests/test_gpu_layer_blocks.py for this comparison); losses finite; every trainable parameter gets a finite gradient, more than
    half of them non-zero; the parameters move."""
    from svol_amd import blocks
    assert blocks.ENABLED
    a = _svanet_step(hidden_dim, 16, per_op=False)
    b = _svanet_step(hidden_dim, 16, per_op=True)
    for r in (a, b):
        assert math.isfinite(r['total']) and all(math.isfinite(v) for v in r['losses'].values()), r['losses']
        assert r['grads'] and all(g is not None and bool(torch.isfinite(g).all()) for g in r['grads'].values())
        assert sum(float(g.abs().max()) > 0 for g in r['grads'].values()) > len(r['grads']) // 2
        assert r['moved'] > len(r['grads']) // 2
    for (la, ba), (lb, bb) in zip(a['outs'], b['outs']):
        assert torch.equal(la, lb) and torch.equal(ba, bb), 'forward outputs differ between the block and the per-op path'
    assert a['total'] == b['total']
