"""CPU-side checks of the C-ABI boundary: the library builds/loads and exports every symbol that
include/svol_hip.h declares (no compute calls without a GPU), and the product refuses to run on CPU."""
import os
import re

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    txt = open(os.path.join(REPO, 'include', 'svol_hip.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    return sorted(set(re.findall(r'\b(svol_[a-z0-9_]+)\s*\(', txt)))


def test_header_symbols_exported():
    from svol_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    L = _lib.lib()
    names = _declared()
    assert len(names) >= 18
    for n in names:
        assert hasattr(L, n), f'{n} declared in include/svol_hip.h but not exported'
    assert set(_lib.SIGNATURES) | {'svol_abi_version', 'svol_strerror', 'svol_block_slot_names'} == set(names)
    # the composite block programs reject null tables before any launch
    for fn in ('svol_video_half_fwd', 'svol_query_self_fwd', 'svol_query_cross_fwd', 'svol_query_cross_wgrad'):
        assert getattr(L, fn)(0, 0, 0) == -1
    for blk, first in ((0, 'X32'), (1, 'O32'), (2, 'O32')):
        assert L.svol_block_slot_names(blk).decode().split(',')[0] == first
    assert L.svol_abi_version() == 7
    assert b'invalid' in L.svol_strerror(-1)


def _host_lsap(cost):
    import ctypes
    import numpy as np
    from svol_amd import _lib
    c = np.ascontiguousarray(cost, dtype=np.float64)
    nr, nc = c.shape
    n = min(nr, nc)
    rows, cols = np.full(max(n, 1), -7, np.int64), np.full(max(n, 1), -7, np.int64)
    rc = _lib.lib().svol_lsap_solve(c.ctypes.data_as(ctypes.c_void_p), nr, nc, rows.ctypes.data_as(ctypes.c_void_p),
                                    cols.ctypes.data_as(ctypes.c_void_p))
    return rc, rows[:n], cols[:n]


def test_host_lsap_known_answers():
    """svol_lsap_solve (host entry of SURVEY §8b, svol_amd/csrc/lsap_host.hip — not the oracle's file) against the scipy 1.15.3
    known answers of tests/golden/lsap_known_answers.npz (ties, zeros, tall / wide / empty, +inf), SURVEY §8c's vectors, live
    random comparisons with scipy incl. heavy ties, and scipy's error conventions (NaN / -inf invalid, all-inf row infeasible)."""
    import numpy as np
    from scipy.optimize import linear_sum_assignment
    z = np.load(os.path.join(REPO, 'tests', 'golden', 'lsap_known_answers.npz'))
    for i in range(int(z['n'])):
        c = z[f'c{i}/cost']
        rc, r, k = _host_lsap(c)
        assert rc == len(z[f'c{i}/rows']), (i, rc)
        assert r.tolist() == z[f'c{i}/rows'].tolist() and k.tolist() == z[f'c{i}/cols'].tolist(), (i, str(z[f'c{i}/kind']))
    for c, rows, cols in [(np.zeros((4, 2)), [0, 1], [0, 1]), (np.zeros((2, 4)), [0, 1], [0, 1]), (np.zeros((3, 3)), [0, 1, 2], [0, 1, 2]),
                          (np.array([[1, 2], [1, 2], [0, 2], [1, 0], [1, 0]], float), [2, 3], [0, 1]),
                          (np.array([[.3, .1], [.1, .3], [.2, .2]], np.float32), [0, 1], [1, 0]),
                          (np.random.default_rng(0).random((10, 3)).astype(np.float32), [1, 3, 4], [0, 2, 1])]:
        rc, r, k = _host_lsap(c)
        assert rc == len(rows) and r.tolist() == rows and k.tolist() == cols
    assert _host_lsap(np.zeros((10, 0)))[0] == 0
    rng = np.random.RandomState(11)
    for it in range(300):
        nr, nc = rng.randint(1, 90), rng.randint(1, 90)
        c = (rng.randint(0, 3, size=(nr, nc)).astype(np.float32) if it % 3 == 0 else rng.random_sample((nr, nc)).astype(np.float32)
             if it % 3 == 1 else rng.standard_normal((nr, nc)))
        rr, cc = linear_sum_assignment(c)
        rc, r, k = _host_lsap(c)
        assert rc == len(rr) and r.tolist() == rr.tolist() and k.tolist() == cc.tolist(), (it, nr, nc)
    bad = np.ones((3, 3))
    bad[1, 1] = np.nan
    assert _host_lsap(bad)[0] == -1
    bad[1, 1] = -np.inf
    assert _host_lsap(bad)[0] == -1
    bad[1, :] = np.inf
    assert _host_lsap(bad)[0] == -2
    ok = np.array([[np.inf, 1.0], [2.0, np.inf], [0.5, 0.25]])
    rr, cc = linear_sum_assignment(ok)
    rc, r, k = _host_lsap(ok)
    assert rc == 2 and r.tolist() == rr.tolist() and k.tolist() == cc.tolist()


def test_argument_validation_without_gpu():
    """Null pointers / bad shapes are rejected before any launch (safe to call without a device)."""
    from svol_amd import _lib
    L = _lib.lib()
    assert L.svol_gemm_nt(0, 8, 0, 0, 0, 8, 0, 8, 0, 0, 0, 0, 0, 0, 0, 0, 4, 4, 8, 1, 0) == -1
    assert L.svol_attn_fwd(0, 8, 0, 8, 0, 8, 0, 8, 0, 0, 1, 1, 1, 1, 8, 1.0, 0.0, 0, 0, 1, 0) == -1
    # few queries: key-split partials; many queries: one int per (batch, 128-key tile) for the masked fast kernels or one per
    # workgroup (batch, head, 128-query tile) for the fast forward's redo flags, whichever is larger
    assert L.svol_attn_ws_bytes(8, 8, 100, 6272, 32) > 8 * 49 * 4 and L.svol_attn_ws_bytes(8, 8, 6272, 6272, 32) == (8 * 6272 * 256 + 64 * 4 * 2 * 128 * 32) * 4   # single-pass backward: fp32 dQ image + tail partials
    assert L.svol_cast(0, 0, 0, 1, 10, 0) == -1


def test_gemm_entries_refuse_before_any_launch():
    """The refusal contract of the five GEMM entry points (csrc/gemm.hip and the 16-bit families behind it), as a table: every call
    below returns before a kernel is launched, and its code is written out.  Non-null operands are small integers used as addresses
    (nothing dereferences them on the host); the grouped records live in a real host array.  Entries that set two faults pin the order
    of precedence.  With a GPU present the test skips itself: an entry that a later change stopped refusing would otherwise launch a
    kernel on a made-up address."""
    if torch.cuda.is_available():
        pytest.skip('made-up addresses: only safe where a launch cannot happen')
    import ctypes
    from svol_amd import _lib
    L = _lib.lib()
    F32, BF16, F16, NODT = 0, 1, 2, 7
    NONE, RELU, GELU, SIGMOID, RELU_RES, GELU_D = 0, 1, 2, 3, 4, 5
    PA, PB, PC, PX, ODD = 0x1000, 0x2000, 0x3000, 0x4000, 0x5008   # ODD: 8 bytes off the 16-byte grid
    BIG = (1 << 30) + 64

    def nt(A=PA, lda=64, A2=0, n_split=0, B=PB, ldb=64, C=PC, ldc=64, bias=0, colscale=0, act=NONE, pre=0, ldp=0, res=0, ldr=0,
           out_f32=0, M=4, N=64, K=64, dtype=BF16):
        return L.svol_gemm_nt(A, lda, A2, n_split, B, ldb, C, ldc, bias, colscale, act, pre, ldp, res, ldr, out_f32, M, N, K, dtype, 0)

    def split(A=PA, lda=64, W=PB, ldw=128, C=PC, ldc=64, bias=0, M=4, N=64, K=64):
        return L.svol_gemm_nt_split(A, lda, W, ldw, C, ldc, bias, M, N, K, 0)

    def dact(A=PA, lda=64, B=PB, ldb=64, C=PC, ldc=64, aux=PX, ldaux=64, act=GELU, colsum=0, M=4, N=64, K=64, dtype=BF16):
        return L.svol_gemm_nt_dact(A, lda, B, ldb, C, ldc, aux, ldaux, act, colsum, M, N, K, dtype, 0)

    def tn(A=PA, lda=64, B=PB, ldb=64, C=PC, ldc=64, colsum=0, Mc=128, N=64, K=64, dtype=BF16):
        return L.svol_gemm_tn(A, lda, B, ldb, C, ldc, colsum, Mc, N, K, dtype, 0)

    def grouped(recs, dtype=BF16, n=None, null=False):   # recs: keyword overrides of one valid record each
        arr = (_lib.TnProblem * max(len(recs), 1))()
        for i, kw in enumerate(recs):
            r = dict(A=PA, lda=64, B=PB, ldb=64, C=PC, ldc=64, colsum=0, Mc=128, N=64, K=64)
            r.update(kw)
            arr[i] = _lib.TnProblem(r['A'], r['lda'], r['B'], r['ldb'], r['C'], r['ldc'], r['colsum'], r['Mc'], r['N'], r['K'])
        return L.svol_gemm_tn_grouped(0 if null else ctypes.cast(arr, ctypes.c_void_p), len(recs) if n is None else n, dtype, 0)

    table = [
        # svol_gemm_nt: null operands, negative sizes, K <= 0
        (nt, dict(A=0), -1), (nt, dict(B=0), -1), (nt, dict(C=0), -1), (nt, dict(M=-1), -1), (nt, dict(N=-1), -1),
        (nt, dict(K=0), -1), (nt, dict(K=-8), -1),
        # GELU_D without `pre` (before the empty product), the empty product (before the dtype), an unknown dtype (before the grid)
        (nt, dict(act=GELU_D), -1), (nt, dict(act=GELU_D, M=0), -1), (nt, dict(M=0), 0), (nt, dict(N=0), 0),
        (nt, dict(M=0, dtype=NODT), 0), (nt, dict(dtype=NODT), -1), (nt, dict(dtype=NODT, K=60), -1),
        # K / leading dimensions off the 16-byte grid (before pointer alignment), per element size
        (nt, dict(K=60), -2), (nt, dict(lda=60), -2), (nt, dict(ldb=60), -2), (nt, dict(K=60, dtype=F16), -2),
        (nt, dict(K=6, dtype=F32), -2), (nt, dict(lda=6, dtype=F32), -2), (nt, dict(K=60, A=ODD), -2),
        # misaligned pointers; A2 / n_split
        (nt, dict(A=ODD), -1), (nt, dict(B=ODD), -1), (nt, dict(A=ODD, dtype=F32), -1), (nt, dict(A2=ODD, n_split=128), -1),
        (nt, dict(A2=PX, n_split=64), -2), (nt, dict(A2=ODD, n_split=64), -1), (nt, dict(A2=PX, n_split=64, dtype=F32), -2),
        # sizes above 2^30; more row tiles than a grid takes
        (nt, dict(M=BIG), -2), (nt, dict(N=BIG), -2), (nt, dict(K=BIG), -2), (nt, dict(M=BIG, dtype=F32), -2),
        (nt, dict(M=128 * 65535 + 1), -2), (nt, dict(M=128 * 65535 + 1, dtype=F32), -2),
        # svol_gemm_nt_split: K <= 0 or off the grid is `unsupported` (before the null check), the rest as svol_gemm_nt
        (split, dict(K=0), -2), (split, dict(K=-8), -2), (split, dict(K=12), -2), (split, dict(K=0, A=0), -2), (split, dict(A=0), -1),
        (split, dict(W=0), -1), (split, dict(C=0), -1), (split, dict(M=-1), -1), (split, dict(M=0), 0), (split, dict(N=0), 0),
        (split, dict(lda=60), -2), (split, dict(ldw=124), -2), (split, dict(A=ODD), -1), (split, dict(W=ODD), -1),
        (split, dict(M=BIG), -2), (split, dict(N=BIG), -2),
        # svol_gemm_nt_dact: null operands (aux among them), sizes, the activations it does not take (before the empty product)
        (dact, dict(A=0), -1), (dact, dict(B=0), -1), (dact, dict(C=0), -1), (dact, dict(aux=0), -1), (dact, dict(M=-1), -1),
        (dact, dict(N=-1), -1), (dact, dict(K=0), -1), (dact, dict(act=NONE), -1), (dact, dict(act=SIGMOID), -1),
        (dact, dict(act=RELU_RES), -1), (dact, dict(act=9), -1), (dact, dict(act=NONE, M=0), -1), (dact, dict(M=0), 0),
        (dact, dict(N=0, act=RELU), 0), (dact, dict(M=0, dtype=NODT, colsum=PX), 0),
        # what no fused kernel takes ends in the generic composition: dense C / aux first, then svol_gemm_nt's own checks
        (dact, dict(A=ODD), -1), (dact, dict(A=ODD, ldc=128), -2), (dact, dict(A=ODD, ldaux=128), -2), (dact, dict(K=60), -2),
        (dact, dict(lda=60, act=GELU_D), -2), (dact, dict(dtype=NODT), -1), (dact, dict(dtype=NODT, ldc=128), -2),
        (dact, dict(K=6, dtype=F32), -2), (dact, dict(A=ODD, dtype=F32), -1), (dact, dict(M=BIG, dtype=F32), -2),
        (dact, dict(M=BIG), -2), (dact, dict(K=60, dtype=F16, colsum=PX), -2),
        # svol_gemm_tn: N = 0 is invalid here, Mc = 0 is the empty product (before the dtype)
        (tn, dict(A=0), -1), (tn, dict(B=0), -1), (tn, dict(C=0), -1), (tn, dict(Mc=-1), -1), (tn, dict(N=0), -1), (tn, dict(K=0), -1),
        (tn, dict(K=-8), -1), (tn, dict(Mc=0), 0), (tn, dict(Mc=0, dtype=NODT), 0), (tn, dict(dtype=NODT), -1),
        (tn, dict(N=60), -2), (tn, dict(K=60), -2), (tn, dict(lda=60), -2), (tn, dict(ldb=60), -2), (tn, dict(K=60, A=ODD), -2),
        (tn, dict(A=ODD), -1), (tn, dict(B=ODD), -1), (tn, dict(Mc=BIG), -2), (tn, dict(N=BIG), -2), (tn, dict(K=BIG), -2),
        (tn, dict(N=6, dtype=F32), -2), (tn, dict(A=ODD, dtype=F32), -1), (tn, dict(N=BIG, dtype=F32), -2), (tn, dict(K=60, dtype=F16), -2),
        # svol_gemm_tn_grouped: the array and the count, then each record's own refusal (issued one by one when the group does not fit)
        (grouped, dict(recs=[{}, {}], null=True), -1), (grouped, dict(recs=[{}, {}], n=-1), -1), (grouped, dict(recs=[{}, {}], dtype=NODT), -1),
        (grouped, dict(recs=[], n=0), 0), (grouped, dict(recs=[dict(A=0), {}]), -1), (grouped, dict(recs=[dict(Mc=0), dict(K=0)]), -1),
        (grouped, dict(recs=[dict(A=ODD), dict(A=ODD)]), -1), (grouped, dict(recs=[dict(N=12), dict(N=12)]), -2),
        (grouped, dict(recs=[dict(N=6), dict(N=6)], dtype=F32), -2), (grouped, dict(recs=[dict(B=ODD)], dtype=F32), -1),
        (grouped, dict(recs=[dict(Mc=BIG), dict(Mc=BIG)], dtype=F16), -2),
    ]
    got = [(fn.__name__, kw, fn(**kw)) for fn, kw, _ in table]
    assert got == [(fn.__name__, kw, rc) for fn, kw, rc in table]
    assert len(table) == 112


def test_attention_scratch_queries_agree_with_the_dispatch_twin():
    """The launch plan of csrc/attention_bf16.hip (attn_plan) and its twin (tests/attn_range_cases.py) are held together through the
    two exported scratch queries, over a grid of shapes: svol_attn_ws_bytes is the twin's ws_floats, and with that much scratch the
    single-pass image (svol_attn_bwd_sp_image_bytes) is there exactly when the twin's shape test holds and the scratch covers the
    single pass's need; one float less than that need and the image is gone."""
    if 'SVOL_DETERMINISTIC' in os.environ:
        pytest.skip('SVOL_DETERMINISTIC is set: the library reads it once and it changes the single-pass shapes')
    import itertools
    from svol_amd import _lib
    from tests import attn_range_cases as A
    L = _lib.lib()
    lens = (1, 70, 100, 128, 129, 200, 256, 384, 640, 1024, 1100, 1152, 2048, 6272, 8400)
    n = images = 0
    for B, H, Lq, Lk, dh in itertools.product((1, 2, 3, 8), (1, 4, 8, 16), lens, lens, (8, 16, 32, 40, 64)):
        dims = (B, H, Lq, Lk, dh)
        ws = int(L.svol_attn_ws_bytes(*dims))
        assert ws == 4 * A.ws_floats(*dims), dims
        if dh > 32:   # csrc/attention.hip's generic kernels at two d-tiles: no scratch, no single-pass image, whatever the scratch
            assert ws == 0 and int(L.svol_attn_bwd_sp_image_bytes(*dims, 1 << 30, 1)) == 0, dims
            assert A.plan(*dims, True, False) == dict(fwd='wide', bwd='wide', ksplit=1, tps=A.cdiv(Lk, A.KT), head_xcd=0), dims
        sp = 4 * A.sp_ws_floats(B, H, Lq, Lk)
        want = B * Lq * H * 32 * 4 if A.sp_shape_ok(*dims) and ws >= sp else 0
        assert int(L.svol_attn_bwd_sp_image_bytes(*dims, ws, 1)) == want, dims   # (1: SVOL_BF16)
        if want:
            assert int(L.svol_attn_bwd_sp_image_bytes(*dims, sp - 4, 1)) == 0, dims
            images += 1
        n += 1
    assert n == 18000 and images > 0


def test_reference_style_cli_trains_the_resnet_backbone_by_default():
    """the reference's shipped runs (train_*.sh: --backbone resnet; train.py:72 optimises every parameter under
    model.train(); its --freeze_backbone is parsed and never read) train the backbone.  A reference command line through
    svol_amd.configs + build_model must therefore build TRAINABLE extractors by default; --freeze_backbone (honoured here) and
    --train_backbone 0 select the frozen ones; --sync_bn reaches the extractors (train.py:65-68)."""
    from svol_amd import configs
    from svol_amd.modeling.model import build_model
    base = ['--backbone', 'resnet', '--num_layers', '1', '--num_queries', '10', '--matcher', 'video_matcher']
    for argv, want_train, want_sync in [(base, True, False), (base + ['--freeze_backbone'], False, False),
                                        (base + ['--train_backbone', '0'], False, False),
                                        (base + ['--freeze_backbone', '--train_backbone', '1', '--sync_bn'], True, True)]:
        args = configs.parse_args(argv)
        model = build_model(args)
        bb = list(model.backbone.parameters())
        assert len(bb) == 108 + 60
        assert all(p.requires_grad == want_train for p in bb), argv
        assert model.backbone.video_backbone.trainable == want_train and model.backbone.sketch_backbone.trainable == want_train
        assert model.backbone.video_backbone.sync_bn == want_sync and model.backbone.sketch_backbone.sync_bn == want_sync
        n_opt = sum(1 for p in model.parameters() if p.requires_grad)   # train.py:72's list
        assert n_opt == sum(1 for p in model.head.parameters() if p.requires_grad) + (len(bb) if want_train else 0)


def test_product_has_no_cpu_path():
    from svol_amd import synthetic as syn
    from svol_amd.modeling.loss import build_loss
    from svol_amd.modeling.svanet import build_svanet
    a = syn.head_args(hidden_dim=32, nheads=4, num_layers=1, num_queries=8, num_frames=4, input_vid_dim=32,
                      input_skch_dim=32)
    m = build_svanet(a)
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 1, 32), torch.ones(1, 1), torch.zeros(1, 8, 32), torch.ones(1, 8))
    c = build_loss(a)
    with pytest.raises(RuntimeError):
        c({'pred_logits': torch.zeros(1, 8, 2), 'pred_boxes': torch.rand(1, 8, 4)}, syn.synth_targets(1, 4))


def test_product_never_imports_oracle():
    import subprocess
    import sys
    code = ('import sys; import svol_amd, svol_amd.ops, svol_amd.modeling.model, svol_amd.modeling.loss, '
            'svol_amd.configs; assert not any(m == "oracle" or m.startswith("oracle.") for m in sys.modules), '
            '"product imported oracle"')
    subprocess.check_call([sys.executable, '-c', code], cwd=REPO)


def test_state_dict_keys_match_reference():
    from svol_amd import synthetic as syn
    from svol_amd.modeling.svanet import build_svanet
    from tests.helpers import load_golden
    z, meta = load_golden('head_mid_video')
    a = syn.head_args(**meta['args'])
    m = build_svanet(a)
    assert list(m.state_dict().keys()) == str(z['keys']).split('\n')


def test_option_surface_defaults():
    import json
    from svol_amd import configs
    ref = json.load(open(os.path.join(REPO, 'tests', 'golden', 'configs_defaults.json')))
    assert configs.reference_defaults() == ref
    a = configs.parse_args(['--num_layers', '6', '--matcher', 'video_matcher', '--num_queries', '100'])
    assert a.num_layers == 6 and a.matcher == 'video_matcher' and a.compute_dtype == 'bf16'


def test_driver_build_entry_agrees_with_the_library_version():
    """__graft_entry__.build() asserts the ABI version it was written against: keep it in step with svol_abi_version()."""
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), '__graft_entry__.py')).read()
    m = re.search(r'svol_abi_version\(\) == (\d+)', src)
    assert m, 'no ABI assertion in __graft_entry__.build()'
    from svol_amd import _lib
    assert int(m.group(1)) == _lib.lib().svol_abi_version()
