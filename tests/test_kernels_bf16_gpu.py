"""Per-kernel parity of the bf16 build: every case of the kernel files (tests/test_kernels_gpu.py, tests/test_text_kernels_gpu.py,
tests/test_optim_rng_gpu.py, tests/test_kernel_contracts_gpu.py, tests/test_autotune_variants_gpu.py) against
libvneti_hip_bf16.so.

A process computes in ONE 16-bit format (view_neti_amd/lib.py), so the bf16 run of the kernel file is a child pytest
process with VNETI_PRECISION=bf16, one per GROUP of the file (so that a failure names its area and each child has a time
limit of its own; a group belongs to one file).  tests/test_bf16_gpu.py checks whole bf16 train steps against the oracle,
with bars that see an O(1) error; here every tile hint, conv K order, split-K path, norm shape, attention head dim and elementwise kernel of the bf16
machine code is compared with its fp32 reference at the fp16 tolerance times 8 (see the kernel file's docstring).

What a parent test asserts from the child's junit report: errors = 0, failures = 0, SKIPPED = 0 and tests run == the
number the same `-k` expression collects — a child that found no GPU (everything skipped), a typo in `-k` (nothing
selected) or a crash halfway cannot pass as "0 failed".  `test_groups_cover_the_kernel_file` proves, for every kernel file,
that its groups are disjoint and that their union is the file's whole collection, so no kernel test is left out of the bf16 run.

Shared-machine shape: the children run one at a time (parent + one child on the GPU, never more), each under its own
time limit; nothing is retried; once a child has died (signal, abort, time limit) the remaining groups FAIL at once
without starting a process — a GPU that has just faulted is not handed further work."""
import os
import subprocess
import sys
import time
import xml.etree.ElementTree as ET

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL_FILE = os.path.join("tests", "test_kernels_gpu.py")
TEXT_FILE = os.path.join("tests", "test_text_kernels_gpu.py")
OPTIM_RNG_FILE = os.path.join("tests", "test_optim_rng_gpu.py")
CONTRACTS_FILE = os.path.join("tests", "test_kernel_contracts_gpu.py")
VARIANTS_FILE = os.path.join("tests", "test_autotune_variants_gpu.py")

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
}
# kernel file -> the least number of cases its collection must hold (a file that lost its tests cannot pass as "covered")
KERNEL_FILES = {KERNEL_FILE: 500, TEXT_FILE: 120, OPTIM_RNG_FILE: 30, CONTRACTS_FILE: 100, VARIANTS_FILE: 11}
DEATH_CODES = (124, 134, 137, 139)  # time limit, abort, kill, segmentation fault (a negative code is a signal)

_dead = None        # "group X died with rc N": set once, read by every later group
_collected = {}     # (kernel file, `-k` expression (None: the whole file)) -> collected test ids


def _pytest_cmd(path, *extra):
    return [sys.executable, "-m", "pytest", path, "-m", "gpu", "-q", "-p", "no:cacheprovider", *extra]


def _env():
    return dict(os.environ, VNETI_PRECISION="bf16")  # added to the inherited environment, nothing removed


def _collect(path, expr=None):
    """ids `--collect-only` lists (touches no GPU: the kernel files import view_neti_amd.ops lazily)"""
    if (path, expr) not in _collected:
        r = subprocess.run(_pytest_cmd(path, "--collect-only", *(["-k", expr] if expr else [])), cwd=ROOT, env=_env(),
                           capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, \
            f"collecting {path} {expr!r} failed (rc {r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}"
        _collected[(path, expr)] = [line.strip() for line in r.stdout.splitlines() if "::" in line]
    return _collected[(path, expr)]


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
    global _dead
    assert _dead is None, f"not run: {_dead}"
    path, expr, limit = GROUPS[group]
    n_collected = len(_collect(path, expr))
    assert n_collected > 0
    xml = tmp_path / "junit.xml"
    t0 = time.time()
    try:
        r = subprocess.run(_pytest_cmd(path, "-k", expr, f"--junitxml={xml}"), cwd=ROOT, env=_env(), capture_output=True, text=True,
                           timeout=limit)
    except subprocess.TimeoutExpired as e:
        _dead = f"group {group} died with rc TimeoutExpired ({limit} s)"
        out = e.stdout.decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or "")
        raise AssertionError(f"bf16 {group}: no end after {limit} s\n{out[-3000:]}")
    rc, tail = r.returncode, (r.stdout[-6000:] + "\n" + r.stderr[-2000:])
    print(f"[bf16 kernels] group {group}: rc {rc}, {n_collected} collected, {time.time() - t0:.1f} s")
    if rc < 0 or rc in DEATH_CODES:
        _dead = f"group {group} died with rc {rc}"
        raise AssertionError(f"bf16 {group}: the child died with rc {rc}\n{tail}")
    assert xml.exists(), f"bf16 {group}: no junit report (rc {rc})\n{tail}"
    suite = ET.parse(xml).getroot()
    suite = suite if suite.tag == "testsuite" else suite.find("testsuite")
    tests, errors, failures, skipped = (int(suite.get(k, 0)) for k in ("tests", "errors", "failures", "skipped"))
    bad = [f"{c.get('classname')}::{c.get('name')} ({kind})" for c in suite.iter("testcase")
           for kind in ("failure", "error", "skipped") if c.find(kind) is not None]
    print(f"[bf16 kernels] group {group}: {tests} run, {failures} failed, {errors} errors, {skipped} skipped")
    assert errors == 0 and failures == 0 and skipped == 0, \
        f"bf16 {group}: {failures} failed, {errors} errors, {skipped} skipped of {tests}:\n" + "\n".join(bad[:60]) + "\n" + tail
    assert tests == n_collected, f"bf16 {group}: {tests} tests ran, `-k {expr}` collects {n_collected}\n{tail}"
    assert rc == 0, f"bf16 {group}: rc {rc}\n{tail}"
