"""The enc/dec Transformer and the heads on it (svanet_variants, SketchDETR) inside a captured graph at --dropout 0.1: every replay
draws fresh masks, and a replay draws the masks of the EAGER step with the same step number (the device-side step counter of
Transformer.step_dev / _DetrHead.step_dev, advanced inside the graph), so a checkpoint continues the mask stream in either direction.

Bars, relative to max |reference| (the reference is an eager twin: same weights, same kernels, the step number set by hand):
fp32 1e-5 -- only the order of atomic sums may differ --, bf16 1e-2, the project's bf16 bar.  A twin ONE step off must miss by more
than 10 x the bar, so that the bar cannot hide a wrong step number; that the tiny case's seed and inputs give such a margin is checked
on the CPU (oracle/encdec_oracle.py under the numpy twin's masks) by the one test here that needs no GPU.

A captured svol_cast_transpose_multi reads the weight cache's descriptor table through the pointer it had at capture time, and the
table is rebuilt when a weight is registered or dies: every model of a test is therefore built, and run once, BEFORE the capture.
"""
from __future__ import annotations

import gc
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.dropout_twin import dropout_keep_numpy

gpu = pytest.mark.gpu
BAR = {'fp32': 1e-5, 'bf16': 1e-2}
WARMUP = 3

# ----------------------------------------------------------------------------------------------------------------------
# the tiny Transformer
# ----------------------------------------------------------------------------------------------------------------------
D, H, F, B, L, N, PAD, P_DROP, BASE_SEED = 32, 4, 64, 2, 40, 8, 7, 0.1, 1
TINY_ARGS = SimpleNamespace(nheads=H, pre_norm=False, enc_layers=1, dec_layers=1)


def _build_tiny(dtype):
    from svol_amd.modeling.transformer import Transformer
    return Transformer(d_model=D, nhead=H, num_encoder_layers=1, num_decoder_layers=1, dim_feedforward=F, dropout=P_DROP,
                       compute_dtype=dtype)


def tiny_case():
    """weights (synthetic.synth_like: every bias and LayerNorm parameter non-trivial), inputs and the probe of the tiny case, on the CPU"""
    from svol_amd import synthetic as syn
    sd = syn.synth_like({k: v.shape for k, v in _build_tiny('fp32').state_dict().items()}, seed=5)
    g = torch.Generator().manual_seed(11)
    src = torch.randn((B, L, D), generator=g)
    pos = 0.5 * torch.randn((B, L, D), generator=g)
    query = torch.randn((N, D), generator=g)
    mask = torch.zeros((B, L), dtype=torch.bool)
    mask[1, L - PAD:] = True
    probe = syn.synth_probe((1, B, N, D), 'hs')
    return sd, src, mask, query, pos, probe


def twin_masks(step):
    """the keep masks (scaled) of training step `step` from the numpy twin, in the oracle's call order"""
    seed0 = (BASE_SEED << 44) + (step << 12)

    def m(shape, seed):
        return torch.from_numpy(dropout_keep_numpy(shape, P_DROP, seed)).float() / (1.0 - P_DROP)
    e, d = seed0 + (0 << 4), seed0 + (64 << 4)
    return [m((B, H, L, L), e + 0), m((B, L, D), e + 1), m((B, L, F), e + 4), m((B, L, D), e + 5),
            m((B, H, N, N), d + 0), m((B, N, D), d + 1), m((B, H, N, L), d + 2), m((B, N, D), d + 3), m((B, N, F), d + 4), m((B, N, D), d + 5)]


def test_neighbouring_steps_of_the_tiny_case_are_far_apart_in_the_oracle():
    """steps 4 .. 7 (the replays behind three warm-ups, and their neighbours): hs under the twin's masks of step s and of s + 1 differ
    by more than 10 x the bf16 bar -- with margin 2, for the device's own bf16 error -- relative to max |hs|"""
    from oracle import encdec_oracle as E
    sd, src, mask, query, pos, _ = tiny_case()
    hs = {}
    for s in range(WARMUP + 1, WARMUP + 5):
        feed = E.MaskFeed(twin_masks(s))
        hs[s] = E.transformer_forward(sd, '', TINY_ARGS, src, mask, query, pos, drop=feed)[0]
        assert feed.i == 10
    for s in range(WARMUP + 1, WARMUP + 4):
        miss = float((hs[s] - hs[s + 1]).abs().max() / hs[s].abs().max())
        print(f'oracle, steps {s} / {s + 1}: hs differs by {miss:.3f} of max |hs|')
        assert miss > 2 * 10 * BAR['bf16'], (s, miss)


def _rel(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max() / ref.abs().max()) if bool(torch.isfinite(got).all()) else float('inf')


@gpu
@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_tiny_transformer_replays_draw_the_eager_steps_masks(dtype):
    gc.collect()
    sd, src, mask, query, pos, probe = (t.cuda() if torch.is_tensor(t) else t for t in tiny_case())
    model, twin = _build_tiny(dtype), _build_tiny(dtype)
    for m in (model, twin):
        m.load_state_dict(sd)
        m.cuda().train()
        m.drop_base_seed = BASE_SEED
    params, tparams = list(model.parameters()), list(twin.parameters())

    def eager_twin(step):
        twin.load_dropout_state({'drop_base_seed': BASE_SEED, 'drop_step': step - 1})
        hs = twin(src, mask, query, pos, need_weights=False)[0]
        return hs.detach(), torch.autograd.grad((hs * probe).sum(), tparams, allow_unused=True)

    eager_twin(1)   # (registers the twin's weight copies before the capture)
    counter = model.step_dev = torch.zeros((1,), dtype=torch.int64, device='cuda')

    def step():
        counter.add_(1)
        hs = model(src, mask, query, pos, need_weights=False)[0]
        return hs, torch.autograd.grad((hs * probe).sum(), params, allow_unused=True)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(WARMUP):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s_hs, s_grads = step()
    torch.cuda.synchronize()
    assert int(counter) == WARMUP and model._drop_step == 0          # the capture ran nothing; the host step stands still
    bar = BAR[dtype]
    for r in range(1, 4):
        graph.replay()
        torch.cuda.synchronize()
        eff = model.dropout_state()['drop_step']
        assert eff == WARMUP + r == int(counter)
        hs, grads = s_hs.clone(), [g.clone() if g is not None else None for g in s_grads]
        ref_hs, ref_grads = eager_twin(eff)
        off_hs, _ = eager_twin(eff + 1)
        e, off = _rel(hs, ref_hs), _rel(hs, off_hs)
        print(f'tiny {dtype} replay {r} (step {eff}): hs {e:.3e} of max |hs| (bar {bar:.0e}); the twin one step off misses by {off:.3e}')
        assert e <= bar, (r, e)
        assert off > 10 * bar, (r, off)
        if dtype == 'fp32':
            worst = 0.0
            for (n, _), g, rg in zip(model.named_parameters(), grads, ref_grads):
                assert (g is None) == (rg is None), n
                if g is not None:
                    worst = max(worst, _rel(g, rg))
            print(f'tiny fp32 replay {r}: worst parameter gradient {worst:.3e} of its max (bar {bar:.0e})')
            assert worst <= bar, (r, worst)


# ----------------------------------------------------------------------------------------------------------------------
# GraphedTrainStep over the heads
# ----------------------------------------------------------------------------------------------------------------------
HEADS = ['append_to_seq', 'concat_to_qry', 'sketch_detr']
KEYS = ('src_sketch', 'src_sketch_mask', 'src_video', 'src_video_mask')


def _head_setup(head, dtype):
    """(args, build, inputs on the device, targets) of one head at B = 2, T = 4, L = 16"""
    from svol_amd import synthetic as syn
    from svol_amd.modeling.sketch_detr import build_sketchdetr
    from svol_amd.modeling.svanet_variants import build_svanet
    Bh, T, Lh = 2, 4, 16
    if head == 'sketch_detr':
        args = syn.encdec_args(dropout=0.1, sketch_head='sketch_detr', mode='unused', matcher='video_matcher', num_layers=2, num_frames=T)
        build, inp = build_sketchdetr, syn.synth_encdec_inputs(args, Bh, T, 1, seed=2)        # one feature per frame
    else:
        args = syn.encdec_args(dropout=0.1, mode=head, matcher='video_matcher', num_layers=2, num_frames=T)
        build, inp = build_svanet, syn.synth_encdec_inputs(args, Bh, Lh, 1, seed=2, pad=3)
    assert args.input_dropout > 0.0
    args.compute_dtype = dtype
    return args, build, {k: v.cuda() for k, v in inp.items()}, syn.synth_targets(Bh, T, seed=2)


def _total(ld, w):
    if isinstance(ld, list):
        return sum(_total(d, w) for d in ld)
    return sum(ld[k] * w[k] for k in ld if k in w)


def _loss_vector(ld, w):
    """the weighted-in entries of a loss dict (or of the list of per-frame dicts), in a fixed order"""
    dicts = ld if isinstance(ld, list) else [ld]
    return torch.stack([d[k].detach().float() for d in dicts for k in sorted(d) if k in w]).cpu()


class _Rig:
    """a head in a GraphedTrainStep (FlatAdamW, capturable, lr = 0 and wd = 0: the weights stand still) and its eager twin"""

    def __init__(self, head, dtype):
        from svol_amd import parallel
        from svol_amd.graph import GraphedTrainStep
        from svol_amd.modeling.loss import build_loss
        gc.collect()
        self.args, build, self.inp, self.tg = _head_setup(head, dtype)
        torch.manual_seed(1)
        self.model = build(self.args).cuda().train()
        self.crit = build_loss(self.args).cuda().train()
        self.twin = build(self.args).cuda().train()
        self.twin_crit = build_loss(self.args).cuda().train()
        self.red = parallel.BucketedGradAllReduce(parallel.arrival_order(self.model), skip=parallel.unused_parameters(self.model), ordered=True)
        self.opt = parallel.FlatAdamW(self.red, lr=0.0, weight_decay=0.0, params=[p for p in self.model.parameters() if p.requires_grad],
                                      capturable=True)
        self.twin.load_state_dict(self.model.state_dict())
        self.eager(1)   # (registers the twin's weight copies before the capture)
        self.gstep = GraphedTrainStep(self.model, self.crit, self.opt, self.red, self.inp, self.tg, warmup=WARMUP)
        assert self.model.step_dev is self.model.transformer.step_dev and self.model._step == 0 and self.model.transformer._drop_step == 0

    def eager(self, step, model=None):
        """the eager step number `step` of the twin (or of `model`): (total loss, loss vector)"""
        m = self.twin if model is None else model
        m._step = step - 1
        m.transformer.load_dropout_state({'drop_base_seed': m.transformer.drop_base_seed, 'drop_step': step - 1})
        with torch.no_grad():
            ld = self.twin_crit(m(*(self.inp[k] for k in KEYS)), self.tg)
        w = self.twin_crit.weight_dict
        return float(_total(ld, w)), _loss_vector(ld, w)

    def replay(self):
        loss, ld = self.gstep(self.inp, self.tg)
        torch.cuda.synchronize()
        return float(loss), _loss_vector(ld, self.crit.weight_dict)


def _hold(what, got, ref, bar):
    (gl, gv), (rl, rv) = got, ref
    e_tot = abs(gl - rl) / abs(rl)
    e_vec = float((gv.double() - rv.double()).abs().max() / rv.double().abs().max())
    print(f'{what}: total loss {gl:.6f} against {rl:.6f} ({e_tot:.3e}), entries {e_vec:.3e} of the largest (bar {bar:.0e})')
    assert gv.shape == rv.shape and bool(torch.isfinite(gv).all())
    assert e_tot <= bar and e_vec <= bar, (what, e_tot, e_vec)


@gpu
@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
@pytest.mark.parametrize('head', HEADS)
def test_graphed_train_step_over_the_encdec_heads(head, dtype):
    rig = _Rig(head, dtype)
    bar = BAR[dtype]
    live = [p for b in rig.red.buckets for p in b['params']]
    before = [p.detach().clone() for p in live]
    losses = []
    for r in range(1, 4):
        got = rig.replay()
        eff = rig.model.transformer.dropout_state()['drop_step']
        assert eff == WARMUP + r
        _hold(f'{head} {dtype} replay {r} (step {eff})', got, rig.eager(eff), bar)
        losses.append(got[0])
    assert len(set(losses)) == 3, losses                                   # fresh masks on every replay
    if dtype == 'fp32':
        assert min(abs(a - b) / abs(a) for a, b in zip(losses, losses[1:])) > 10 * bar, losses
    assert all(torch.equal(a, p.detach()) for a, p in zip(before, live))   # lr = 0, wd = 0: nothing moved
    for g in rig.opt.param_groups:
        g['lr'] = 1e-3
    loss, _ = rig.replay()
    moved = [not torch.equal(a, p.detach()) for a, p in zip(before, live)]
    assert np.isfinite(loss) and sum(moved) > len(moved) // 2, (loss, sum(moved), len(moved))


@gpu
def test_checkpoint_continues_the_mask_stream_of_a_captured_run(tmp_path):
    """n captured steps, save_checkpoint, load into a fresh eager model: its next step draws the masks of step n + 1 -- the graph's next
    replay.  (The head keeps no dropout state of its own: its _step is the checkpoint's step, set by the rig as a driver would.)"""
    from svol_amd.utils.checkpoint import load_checkpoint, save_checkpoint
    rig = _Rig('append_to_seq', 'fp32')
    fresh = rig.twin                      # built and run once before the capture; every weight and counter is overwritten below
    with torch.no_grad():
        for p in fresh.parameters():
            p.zero_()
    fresh.transformer.load_dropout_state({'drop_base_seed': 1, 'drop_step': 0})
    for _ in range(2):
        rig.replay()
    n = WARMUP + 2
    path = save_checkpoint(str(tmp_path / 'graph.ckpt'), rig.model, None, None, n, rig.args)
    _, info = load_checkpoint(path, fresh, resume_all=True)
    assert fresh.transformer.dropout_state() == {'drop_base_seed': 1, 'drop_step': n} and info['start_iter'] == n + 1
    fresh._step = n
    fresh.train()
    with torch.no_grad():
        ld = rig.twin_crit(fresh(*(rig.inp[k] for k in KEYS)), rig.tg)
    w = rig.twin_crit.weight_dict
    ref = (float(_total(ld, w)), _loss_vector(ld, w))
    assert fresh.transformer._drop_step == n + 1
    _hold(f'checkpoint at step {n}: the eager step {n + 1} against the next replay', rig.replay(), ref, BAR['fp32'])
