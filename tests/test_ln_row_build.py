"""The LayerNorm kernels of csrc/norm.hip and csrc/gate.hip compile for gfx950 into their full instance sets -- ln_fwd_kernel /
lnw_fwd_kernel, ln_bwd_kernel at every (T, TX, NP, WPR) (the shared row of csrc/ln_row.h), gate_apply_kernel, ln_scores_kernel (the
shared forward row) and gate_bwd_ln_kernel -- each free of register spills and scratch and at exactly the static LDS its code implies,
and the library build watches the header."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Itanium names of the element types: float, __bf16, _Float16
TYPES = ('f', 'DF16b', 'DF16_')
# (T, TX) of the LayerNorm kernels: fp32 rows under every output type, 16-bit rows under their own
T_TX = {('f', 'f'), ('DF16b', 'f'), ('DF16b', 'DF16b'), ('DF16_', 'f'), ('DF16_', 'DF16_')}
# (NP, WPR): one wave per row at 1, 2, 4 passes of 256 columns; four waves per row at 2, 3, 4 passes of 1024 columns
NP_WPR = {(1, 1), (2, 1), (4, 1), (2, 4), (3, 4), (4, 4)}
LN = {(t, tx, np_, wpr) for t, tx in T_TX for np_, wpr in NP_WPR}


def _hipcc():
    for c in (os.environ.get('HIPCC'), '/opt/rocm/bin/hipcc', shutil.which('hipcc')):
        if c and os.path.exists(c):
            return c
    return None


def _kernels(tmp_path, src):
    """{mangled kernel name: (static LDS, scratch, VGPR spills, SGPR spills)} from the kernel descriptors and the metadata"""
    hipcc = _hipcc()
    if hipcc is None:
        pytest.fail('hipcc not found: the gfx950 build needs it')
    out = tmp_path / (src + '.s')
    subprocess.check_call([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '--cuda-device-only', '-S',
                           os.path.join(REPO, 'svol_amd', 'csrc', src), '-o', str(out)], cwd=REPO)
    asm = out.read_text()
    res = {}
    for k in re.findall(r'\.amdhsa_kernel (\S+)', asm):
        i = asm.index('.amdhsa_kernel ' + k)
        block = asm[i:asm.index('.end_amdhsa_kernel', i)]
        meta = asm[asm.index(f'.name:           {k}\n'):]
        res[k] = (int(re.search(r'\.amdhsa_group_segment_fixed_size (\d+)', block).group(1)),
                  int(re.search(r'\.amdhsa_private_segment_fixed_size (\d+)', block).group(1)),
                  int(re.search(r'\.vgpr_spill_count:\s+(\d+)', meta).group(1)),
                  int(re.search(r'\.sgpr_spill_count:\s+(\d+)', meta).group(1)))
    return res


def _clean(name, k):
    lds, scratch, vspill, sspill = k
    assert scratch == 0 and vspill == 0 and sspill == 0, (name, k)
    return lds


def test_layernorm_kernels_compile_to_the_full_instance_set_without_spills(tmp_path):
    kernels = _kernels(tmp_path, 'norm.hip')
    types = '|'.join(TYPES)
    # forward: ln_fwd_kernel<T, TX, NP> (one wave per row) and lnw_fwd_kernel<T, TX, NV> (four waves per row), their own text
    fwd = {}
    for name, k in kernels.items():
        if 'ln_fwd_kernel' in name or 'lnw_fwd_kernel' in name:
            m = re.search(r'(lnw?)_fwd_kernelI(%s)(%s)Li(\d)EEE' % (types, types), name)
            assert m, name
            fwd[m.group(2), m.group(3), int(m.group(4)), 4 if m.group(1) == 'lnw' else 1] = _clean(name, k)
    assert set(fwd) == LN and len(fwd) == 30, sorted(fwd)
    assert sum('lnw_fwd_kernel' in n for n in kernels) == 15 and sum('ln_fwd_kernel' in n for n in kernels) == 15
    for (t, tx, np_, wpr), lds in fwd.items():   # the row sums of four waves: two sets of four words
        assert lds == (32 if wpr == 4 else 0), (t, tx, np_, wpr, lds)
    # backward: ln_bwd_kernel<T, TX, NP, WPR> on the shared row of ln_row.h
    bwd = {}
    for name, k in kernels.items():
        if 'ln_bwd_kernel' in name:
            m = re.search(r'ln_bwd_kernelI(%s)(%s)Li(\d)ELi(\d)EEE' % (types, types), name)
            assert m, name
            bwd[m.group(1), m.group(2), int(m.group(3)), int(m.group(4))] = _clean(name, k)
    assert set(bwd) == LN and len(bwd) == 30, sorted(bwd)
    assert sum(wpr == 1 for _, _, _, wpr in bwd) == 15 and sum(wpr == 4 for _, _, _, wpr in bwd) == 15
    for (t, tx, np_, wpr), lds in bwd.items():   # the column fold [3][NP * 256 * WPR] floats, and four sets of four words at WPR = 4
        assert lds == 3 * np_ * 256 * wpr * 4 + (64 if wpr == 4 else 0), (t, tx, np_, wpr, lds)
    assert bwd['DF16b', 'f', 1, 1] == 3072 and bwd['DF16b', 'f', 2, 4] == 24640


def test_gate_layernorm_kernels_compile_without_spills(tmp_path):
    kernels = _kernels(tmp_path, 'gate.hip')
    types = '|'.join(TYPES)
    apply_, scores, bwd = {}, {}, {}
    for name, k in kernels.items():
        if 'gate_apply_kernel' in name:
            m = re.search(r'gate_apply_kernelI(%s)Li(\d)ELb([01])EEE' % types, name)
            assert m, name
            apply_[m.group(1), int(m.group(2)), int(m.group(3))] = _clean(name, k)
        elif 'ln_scores_kernel' in name:
            m = re.search(r'ln_scores_kernelI(%s)Li(\d)EEE' % types, name)
            assert m, name
            scores[m.group(1), int(m.group(2))] = _clean(name, k)
        elif 'gate_bwd_ln_kernel' in name:
            m = re.search(r'gate_bwd_ln_kernelI(%s)Li(\d)EEE' % types, name)
            assert m, name
            bwd[m.group(1), int(m.group(2))] = _clean(name, k)
    assert set(apply_) == {(t, np_, w) for t in TYPES for np_ in (1, 2, 4) for w in (0, 1)} and len(apply_) == 18
    assert set(scores) == {(t, 1) for t in TYPES} and len(scores) == 3
    assert set(bwd) == {(t, np_) for t in TYPES for np_ in (1, 2, 4)} and len(bwd) == 9
    assert all(lds == 0 for lds in apply_.values()), apply_
    assert all(lds == 0 for lds in scores.values()), scores   # (u[b] sits in dynamic LDS)
    for (t, np_), lds in bwd.items():
        assert lds == 2 * np_ * 256 * 4, (t, np_, lds)           # the column fold of dgamma | dbeta


def test_the_library_build_watches_the_header(monkeypatch, tmp_path):
    """every source is rebuilt when ln_row.h is newer: build() hands it to its staleness check with the other headers"""
    from svol_amd import build
    assert os.path.exists(os.path.join(build.CSRC, 'ln_row.h'))
    seen = []
    monkeypatch.setattr(build, '_stale', lambda target, deps: seen.append((target, list(deps))) or False)
    monkeypatch.setattr(build.subprocess, 'check_call', lambda *a, **k: pytest.fail('nothing is stale: nothing to run'))
    build.build(verbose=False)
    header = os.path.join(build.CSRC, 'ln_row.h')
    for src in ('norm.o', 'gate.o'):
        deps = [d for t, d in seen if t.endswith(os.sep + src)]
        assert deps and header in deps[0], (src, deps)
