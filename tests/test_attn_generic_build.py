"""csrc/attention.hip's generic template compiles for gfx950 with every instance (forward, dQ, dK/dV at <fp32, 1>, <fp32, 2>, <bf16, 2>,
<fp16, 2>; delta x fp32, bf16, fp16) free of register spills and scratch, inside the LDS of two workgroups per CU and at exactly the
LDS sizes its traits give, and is part of the library build."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# bytes of LDS per workgroup by (element bytes, d-tiles): 64-row natural image of 32 ND columns, transposed image of 32 ND rows at a
# stride of 64 elements + 16 bytes; forward = nat + tr + 64 floats, dQ = 2 nat + tr + 64 floats, dK/dV = 2 nat + 2 tr + 128 floats
# (the table in the file's header)
LDS = {(4, 1): dict(fwd=17152, bwd_dq=25344, bwd_dkdv=34304),
       (2, 2): dict(fwd=17664, bwd_dq=25856, bwd_dkdv=35328),
       (4, 2): dict(fwd=34048, bwd_dq=50432, bwd_dkdv=68096)}
ELEM = {'f': 4, 'DF16b': 2, 'DF16_': 2}   # Itanium names of float, __bf16, _Float16
INSTANCES = {('f', 1), ('f', 2), ('DF16b', 2), ('DF16_', 2)}


def _hipcc():
    for c in (os.environ.get('HIPCC'), '/opt/rocm/bin/hipcc', shutil.which('hipcc')):
        if c and os.path.exists(c):
            return c
    return None


def test_generic_attention_is_in_the_library_build():
    from svol_amd import build
    assert 'attention.hip' in build.SOURCES and 'attention.hip' not in build.H16_SOURCES   # one build: a template on the type
    assert 'attention_wide.hip' not in build.SOURCES + build.H16_SOURCES
    assert not os.path.exists(os.path.join(REPO, 'svol_amd', 'csrc', 'attention_wide.hip'))


def test_generic_attention_kernels_compile_without_spills_or_scratch(tmp_path):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.fail('hipcc not found: the gfx950 build needs it')
    out = tmp_path / 'attention.s'
    subprocess.check_call([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '--cuda-device-only', '-S',
                           os.path.join(REPO, 'svol_amd', 'csrc', 'attention.hip'), '-o', str(out)], cwd=REPO)
    asm = out.read_text()
    kernels = [k for k in re.findall(r'\.amdhsa_kernel (\S+)', asm) if 'attn_' in k]
    for kind in ('fwd', 'bwd_dq', 'bwd_dkdv'):
        got = {re.search(r'attn_%s_kernelI(\w+?)Li(\d)EEE' % kind, k).groups() for k in kernels if f'attn_{kind}_kernel' in k}
        assert {(t, int(nd)) for t, nd in got} == INSTANCES, (kind, kernels)
        assert sum(f'attn_{kind}_kernel' in k for k in kernels) == 4, (kind, kernels)
    assert {re.search(r'attn_delta_kernelI(\w+?)EEv', k).group(1) for k in kernels if 'attn_delta_kernel' in k} == set(ELEM), kernels
    assert sum('attn_delta_kernel' in k for k in kernels) == 3 and len(kernels) == 15, kernels
    for k in kernels:
        i = asm.index('.amdhsa_kernel ' + k)
        block = asm[i:asm.index('.end_amdhsa_kernel', i)]
        assert int(re.search(r'\.amdhsa_private_segment_fixed_size (\d+)', block).group(1)) == 0, k
        lds = int(re.search(r'\.amdhsa_group_segment_fixed_size (\d+)', block).group(1))
        # __launch_bounds__(256, 2): two workgroups of a CU share its 160 KiB of LDS
        assert 2 * lds <= 160 * 1024, k
        m = re.search(r'attn_(fwd|bwd_dq|bwd_dkdv)_kernelI(\w+?)Li(\d)EEE', k)
        assert lds == (LDS[ELEM[m.group(2)], int(m.group(3))][m.group(1)] if m else 0), (k, lds)   # (delta: no LDS)
        meta = asm[asm.index(f'.name:           {k}'):]
        assert int(re.search(r'\.vgpr_spill_count:\s+(\d+)', meta).group(1)) == 0, k
        assert int(re.search(r'\.sgpr_spill_count:\s+(\d+)', meta).group(1)) == 0, k
