"""csrc/attention_wide.hip compiles for gfx950 with every instance (forward, delta, dQ, dK/dV x fp32, bf16, fp16) free of register
spills and scratch, inside the LDS of two workgroups per CU, and is part of the library build."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hipcc():
    for c in (os.environ.get('HIPCC'), '/opt/rocm/bin/hipcc', shutil.which('hipcc')):
        if c and os.path.exists(c):
            return c
    return None


def test_wide_attention_is_in_the_library_build():
    from svol_amd import build
    assert 'attention_wide.hip' in build.SOURCES and 'attention_wide.hip' not in build.H16_SOURCES   # one build: a template on the type


def test_wide_attention_kernels_compile_without_spills_or_scratch(tmp_path):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.fail('hipcc not found: the gfx950 build needs it')
    out = tmp_path / 'attention_wide.s'
    subprocess.check_call([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '--cuda-device-only', '-S',
                           os.path.join(REPO, 'svol_amd', 'csrc', 'attention_wide.hip'), '-o', str(out)], cwd=REPO)
    asm = out.read_text()
    kernels = [k for k in re.findall(r'\.amdhsa_kernel (\S+)', asm) if 'attn_wide' in k]
    for name in ('attn_wide_fwd_kernel', 'attn_wide_delta_kernel', 'attn_wide_bwd_dq_kernel', 'attn_wide_bwd_dkdv_kernel'):
        assert sum(name in k for k in kernels) == 3, (name, kernels)   # float, bf16, fp16
    for k in kernels:
        i = asm.index('.amdhsa_kernel ' + k)
        block = asm[i:asm.index('.end_amdhsa_kernel', i)]
        assert int(re.search(r'\.amdhsa_private_segment_fixed_size (\d+)', block).group(1)) == 0, k
        # __launch_bounds__(256, 2): two workgroups of a CU share its 160 KiB of LDS
        assert 2 * int(re.search(r'\.amdhsa_group_segment_fixed_size (\d+)', block).group(1)) <= 160 * 1024, k
        meta = asm[asm.index(f'.name:           {k}'):]
        assert int(re.search(r'\.vgpr_spill_count:\s+(\d+)', meta).group(1)) == 0, k
        assert int(re.search(r'\.sgpr_spill_count:\s+(\d+)', meta).group(1)) == 0, k
