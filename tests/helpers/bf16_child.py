"""Re-run a selection of a test file against libvneti_hip_bf16.so in a child pytest process (a process computes in ONE
16-bit format, view_neti_amd/lib.py), and judge the child by its junit report.

What `judge_report` asserts: the child did not die, errors = 0, failures = 0, SKIPPED = 0 and tests run == the number the
same `-k` expression collects — a child that found no GPU (everything skipped), a typo in `-k` (nothing selected) or a
crash halfway cannot pass as "0 failed".

Shared-machine shape: the children run one at a time (parent + one child on the GPU, never more), each under its own time
limit; nothing is retried; once a child has died (signal, abort, time limit) every later call, from whichever test file,
FAILS at once without starting a process — a GPU that has just faulted is not handed further work.

pytest does not rewrite the asserts of a helper module: every assert here carries its message."""
import os
import subprocess
import sys
import time
import xml.etree.ElementTree as ET

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
DEATH_CODES = (124, 134, 137, 139)  # time limit, abort, kill, segmentation fault (a negative code is a signal)

_dead = None        # "<child> died with rc N": set once, read by every later call
_collected = {}     # (test file, `-k` expression (None: the whole file), extra arguments) -> collected test ids


def pytest_cmd(path, *extra):
    return [sys.executable, "-m", "pytest", path, "-m", "gpu", "-q", "-p", "no:cacheprovider", *extra]


def bf16_env():
    return dict(os.environ, VNETI_PRECISION="bf16")  # added to the inherited environment, nothing removed


def collect(path, expr=None, limit=240, extra_args=()):
    """ids `--collect-only` lists (touches no GPU: the kernel files import view_neti_amd.ops lazily)"""
    key = (path, expr, tuple(extra_args))
    if key not in _collected:
        r = subprocess.run(pytest_cmd(path, *extra_args, "--collect-only", *(["-k", expr] if expr else [])), cwd=ROOT,
                           env=bf16_env(), capture_output=True, text=True, timeout=limit)
        assert r.returncode == 0, \
            f"collecting {path} {expr!r} failed (rc {r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}"
        _collected[key] = [line.strip() for line in r.stdout.splitlines() if "::" in line]
    return _collected[key]


def died(rc):
    return rc < 0 or rc in DEATH_CODES


def judge_report(rc, xml_path, n_collected, expect=None, what="bf16 child", tail=""):
    """pure: the child's return code and junit report against the number of collected (and, if given, expected) cases"""
    assert not died(rc), f"{what}: the child died with rc {rc}\n{tail}"
    assert os.path.exists(xml_path), f"{what}: no junit report (rc {rc})\n{tail}"
    suite = ET.parse(xml_path).getroot()
    suite = suite if suite.tag == "testsuite" else suite.find("testsuite")
    tests, errors, failures, skipped = (int(suite.get(k, 0)) for k in ("tests", "errors", "failures", "skipped"))
    bad = [f"{c.get('classname')}::{c.get('name')} ({kind})" for c in suite.iter("testcase")
           for kind in ("failure", "error", "skipped") if c.find(kind) is not None]
    print(f"[{what}] {tests} run, {failures} failed, {errors} errors, {skipped} skipped")
    assert errors == 0 and failures == 0 and skipped == 0, \
        f"{what}: {failures} failed, {errors} errors, {skipped} skipped of {tests}:\n" + "\n".join(bad[:60]) + "\n" + tail
    assert tests == n_collected, f"{what}: {tests} tests ran, the same selection collects {n_collected}\n{tail}"
    assert expect is None or tests == expect, f"{what}: {tests} tests ran, {expect} expected\n{tail}"
    assert rc == 0, f"{what}: rc {rc}\n{tail}"


def run_bf16_child(path, expr, limit, tmp_path, least, extra_args=(), expect=None, collect_limit=240, what=None):
    """collect `path -k expr` (no GPU), run it in ONE child with VNETI_PRECISION=bf16 under `limit` seconds, judge its
    report -> the child's stdout"""
    global _dead
    what = what or f"bf16 {path} -k {expr!r}"
    assert _dead is None, f"not run: {_dead}"
    n_collected = len(collect(path, expr, collect_limit, extra_args))
    assert n_collected >= least, f"{what}: `-k {expr}` collects {n_collected} cases, at least {least} expected"
    xml = tmp_path / "junit.xml"
    t0 = time.time()
    try:
        r = subprocess.run(pytest_cmd(path, *extra_args, "-k", expr, f"--junitxml={xml}"), cwd=ROOT, env=bf16_env(),
                           capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired as e:
        _dead = f"{what} died with rc TimeoutExpired ({limit} s)"
        out = e.stdout.decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or "")
        raise AssertionError(f"{what}: no end after {limit} s\n{out[-3000:]}")
    rc, tail = r.returncode, (r.stdout[-6000:] + "\n" + r.stderr[-2000:])
    print(f"[{what}] rc {rc}, {n_collected} collected, {time.time() - t0:.1f} s")
    if died(rc):
        _dead = f"{what} died with rc {rc}"
    judge_report(rc, xml, n_collected, expect, what, tail)
    return r.stdout
