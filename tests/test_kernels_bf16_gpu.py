"""Per-kernel parity of the bf16 build: every case of the kernel files (tests/test_kernels_gpu.py, tests/test_text_kernels_gpu.py,
tests/test_optim_rng_gpu.py, tests/test_kernel_contracts_gpu.py, tests/test_autotune_variants_gpu.py,
tests/test_norm_edges_gpu.py, tests/test_conv_edges_gpu.py, tests/test_attn_edges_gpu.py) against
libvneti_hip_bf16.so.

A process computes in ONE 16-bit format (view_neti_amd/lib.py), so the bf16 run of the kernel file is a child pytest
process with VNETI_PRECISION=bf16, one per GROUP of the file (so that a failure names its area and each child has a time
limit of its own; a group belongs to one file).  tests/test_bf16_gpu.py checks whole bf16 train steps against the oracle,
with bars that see an O(1) error; here every tile hint, conv K order, split-K path, norm shape, attention head dim and elementwise kernel of the bf16
machine code is compared with its fp32 reference at the fp16 tolerance times 8 (see the kernel file's docstring).

The child runner is tests/helpers/bf16_child.py, shared with the other files that re-run themselves in bf16.  What it
asserts from the child's junit report: errors = 0, failures = 0, SKIPPED = 0 and tests run == the number the same `-k`
expression collects — a child that found no GPU (everything skipped), a typo in `-k` (nothing selected) or a crash halfway
cannot pass as "0 failed".  `test_groups_cover_the_kernel_file` proves, for every kernel file, that its groups are disjoint
and that their union is the file's whole collection, so no kernel test is left out of the bf16 run.

Shared-machine shape: the children run one at a time (parent + one child on the GPU, never more), each under its own
time limit; nothing is retried; once a child has died (signal, abort, time limit) the remaining groups, and the bf16
children of every other file, FAIL at once without starting a process — a GPU that has just faulted is not handed further
work."""
import os

import pytest

from helpers.bf16_child import collect as _collect, run_bf16_child

KERNEL_FILE = os.path.join("tests", "test_kernels_gpu.py")
TEXT_FILE = os.path.join("tests", "test_text_kernels_gpu.py")
OPTIM_RNG_FILE = os.path.join("tests", "test_optim_rng_gpu.py")
CONTRACTS_FILE = os.path.join("tests", "test_kernel_contracts_gpu.py")
VARIANTS_FILE = os.path.join("tests", "test_autotune_variants_gpu.py")
NORM_EDGES_FILE = os.path.join("tests", "test_norm_edges_gpu.py")
CONV_EDGES_FILE = os.path.join("tests", "test_conv_edges_gpu.py")
ATTN_EDGES_FILE = os.path.join("tests", "test_attn_edges_gpu.py")

# group -> (kernel file, `-k` expression, time limit of the child in seconds).  The limits are several times the wall times
# measured on an MI355X (the tables of the per-kernel parity runs), and never above 300 s.
GROUPS = {
    "gemm": (KERNEL_FILE, "gemm", 120),
    "conv": (KERNEL_FILE, "(conv or im2col) and not gemm", 120),
    "norms": (KERNEL_FILE, "(groupnorm or layernorm or softmax or transpose) and not gemm", 180),
    "attention": (KERNEL_FILE, "attention", 120),
    "elementwise": (KERNEL_FILE, "elementwise or precision", 90),
    "mapper": (TEXT_FILE, "mapper or legacy", 90),
    "text_splice": (TEXT_FILE, "text_embed or text_final or text_cast", 90),
    "optimizer": (OPTIM_RNG_FILE, "adamw", 120),
    "rng": (OPTIM_RNG_FILE, "test_rng or dropout", 150),
    "infer_helpers": (OPTIM_RNG_FILE, "conv1x1 or table_fill", 60),
    "contracts_gemm": (CONTRACTS_FILE, "contract_gemm", 60),
    "contracts_conv": (CONTRACTS_FILE, "contract_conv", 60),
    "contracts_norms": (CONTRACTS_FILE, "contract_norm", 60),
    "contracts_attention": (CONTRACTS_FILE, "contract_attn", 60),
    # every autotuner variant of the engines' own GEMM launches (one child per engine family)
    "variants_unet": (VARIANTS_FILE, "unet", 120),
    "variants_vae": (VARIANTS_FILE, "vae", 60),
    "variants_text": (VARIANTS_FILE, "text", 60),
    # the norm kernels at their edges against float64 (group geometry, capacities, dtype paths, offset-dominated groups)
    "edges_groupnorm": (NORM_EDGES_FILE, "edges_groupnorm", 60),
    "edges_layernorm": (NORM_EDGES_FILE, "edges_layernorm", 60),
    "edges_softmax": (NORM_EDGES_FILE, "edges_softmax", 60),
    # the convolutions at their image edges: bit-exact selector launches, Gaussian parity against float64, the small kernels
    "edges_conv_select": (CONV_EDGES_FILE, "edges_conv_select", 60),
    "edges_conv_parity": (CONV_EDGES_FILE, "edges_conv_parity", 60),
    "edges_conv_small": (CONV_EDGES_FILE, "edges_conv_small", 60),
    # the attention kernels at their tile edges against float64: ragged shapes, the online softmax on staircase data, the
    # query split of dK/dV, the one-launch short backward, refusals
    "edges_attn_ragged": (ATTN_EDGES_FILE, "edges_attn_ragged", 60),
    "edges_attn_softmax": (ATTN_EDGES_FILE, "edges_attn_softmax", 60),
    "edges_attn_qsplit": (ATTN_EDGES_FILE, "edges_attn_qsplit", 60),
    "edges_attn_small": (ATTN_EDGES_FILE, "edges_attn_small", 60),
    "edges_attn_refuse": (ATTN_EDGES_FILE, "edges_attn_refuse", 60),
}
# kernel file -> the least number of cases its collection must hold (a file that lost its tests cannot pass as "covered")
KERNEL_FILES = {KERNEL_FILE: 500, TEXT_FILE: 120, OPTIM_RNG_FILE: 30, CONTRACTS_FILE: 100, VARIANTS_FILE: 11,
                NORM_EDGES_FILE: 140, CONV_EDGES_FILE: 340, ATTN_EDGES_FILE: 250}


def test_groups_cover_the_kernel_file():
    """per kernel file: its groups are pairwise disjoint and their union is exactly the file's collection (needs no GPU)"""
    assert {path for path, _, _ in GROUPS.values()} == set(KERNEL_FILES)
    for path, least in KERNEL_FILES.items():
        everything = _collect(path)
        assert len(everything) > least and len(set(everything)) == len(everything), f"{path}: {len(everything)} cases"
        seen = {}
        for group, (gpath, expr, _) in GROUPS.items():
            if gpath != path:
                continue
            ids = _collect(path, expr)
            assert ids, f"group {group}: `-k {expr}` selects nothing in {path}"
            for i in ids:
                assert i not in seen, f"{i} is in the groups {seen[i]} and {group}"
                seen[i] = group
        missing = sorted(set(everything) - set(seen))
        extra = sorted(set(seen) - set(everything))
        assert not missing and not extra, f"{path}: left out of the bf16 run: {missing[:20]}; not in the file: {extra[:20]}"


@pytest.mark.gpu
@pytest.mark.parametrize("group", list(GROUPS))
def test_kernels_bf16(group, tmp_path):
    path, expr, limit = GROUPS[group]
    run_bf16_child(path, expr, limit, tmp_path, least=1, what=f"bf16 kernels group {group}")
