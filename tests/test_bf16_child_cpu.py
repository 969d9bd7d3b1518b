"""`judge_report` of tests/helpers/bf16_child.py on hand-written junit reports (no GPU, no child process): the logic that keeps
"0 failed" from meaning "nothing ran", and the latch that hands a GPU that has just faulted no further child."""
import subprocess

import pytest

from helpers import bf16_child as BC

CASE = '<testcase classname="tests.test_x" name="test_{i}" time="0.01">{body}</testcase>'


def _report(tmp_path, bodies, root="testsuite", counts=None):
    """a junit file with one testcase per entry of `bodies` ('' passed, or a <failure/>, <error/>, <skipped/> element); the
    suite's counters are derived from the bodies unless `counts` overrides them"""
    n = dict(tests=len(bodies), errors=sum("<error" in b for b in bodies), failures=sum("<failure" in b for b in bodies),
             skipped=sum("<skipped" in b for b in bodies))
    n.update(counts or {})
    suite = ('<testsuite name="pytest" errors="{errors}" failures="{failures}" skipped="{skipped}" tests="{tests}">'.format(**n)
             + "".join(CASE.format(i=i, body=b) for i, b in enumerate(bodies)) + "</testsuite>")
    xml = suite if root == "testsuite" else f"<testsuites>{suite}</testsuites>"
    path = tmp_path / "junit.xml"
    path.write_text('<?xml version="1.0" encoding="utf-8"?>' + xml)
    return path


@pytest.mark.parametrize("root", ["testsuite", "testsuites"])
def test_clean_report_passes(tmp_path, root):
    BC.judge_report(0, _report(tmp_path, [""] * 3, root), 3)
    BC.judge_report(0, _report(tmp_path, [""] * 3, root), 3, expect=3)


def test_everything_skipped_fails(tmp_path):
    """a child that found no GPU: rc 0, every case skipped"""
    xml = _report(tmp_path, ['<skipped message="no GPU in this container"/>'] * 3)
    with pytest.raises(AssertionError, match=r"0 failed, 0 errors, 3 skipped of 3:\ntests\.test_x::test_0 \(skipped\)"):
        BC.judge_report(0, xml, 3)


def test_fewer_tests_than_collected_fails(tmp_path):
    """a crash halfway that still left a report, or a selection that differs from the collected one"""
    with pytest.raises(AssertionError, match="2 tests ran, the same selection collects 3"):
        BC.judge_report(0, _report(tmp_path, [""] * 2), 3)
    with pytest.raises(AssertionError, match="0 tests ran, the same selection collects 3"):
        BC.judge_report(0, _report(tmp_path, []), 3)


@pytest.mark.parametrize("root", ["testsuite", "testsuites"])
def test_one_failure_fails_and_is_named(tmp_path, root):
    xml = _report(tmp_path, ["", '<failure message="assert 1 == 2">trace</failure>', ""], root)
    with pytest.raises(AssertionError, match=r"1 failed, 0 errors, 0 skipped of 3:\ntests\.test_x::test_1 \(failure\)"):
        BC.judge_report(1, xml, 3)
    xml = _report(tmp_path, ['<error message="fixture">trace</error>', ""], root)
    with pytest.raises(AssertionError, match=r"0 failed, 1 errors, 0 skipped of 2:\ntests\.test_x::test_0 \(error\)"):
        BC.judge_report(1, xml, 2)


@pytest.mark.parametrize("rc", [139, 134, 137, 124, -11, -6])
def test_death_code_fails_before_the_report_is_read(tmp_path, rc):
    with pytest.raises(AssertionError, match=f"the child died with rc {rc}"):
        BC.judge_report(rc, tmp_path / "junit.xml", 3)  # no report was written
    with pytest.raises(AssertionError, match=f"the child died with rc {rc}"):
        BC.judge_report(rc, _report(tmp_path, [""] * 3), 3)  # nor does a clean one help


def test_missing_report_fails(tmp_path):
    with pytest.raises(AssertionError, match=r"no junit report \(rc 0\)"):
        BC.judge_report(0, tmp_path / "junit.xml", 3)


def test_nonzero_rc_with_a_clean_report_fails(tmp_path):
    with pytest.raises(AssertionError, match="my child: rc 1\nthe tail"):
        BC.judge_report(1, _report(tmp_path, [""] * 3), 3, what="my child", tail="the tail")


def test_expected_count_is_pinned(tmp_path):
    with pytest.raises(AssertionError, match="3 tests ran, 4 expected"):
        BC.judge_report(0, _report(tmp_path, [""] * 3), 3, expect=4)


def test_after_a_death_no_further_child_is_started(tmp_path, monkeypatch):
    """the latch is the module's, so it holds across test files; a child that runs out of time sets it"""
    calls = []

    def run(cmd, **kw):
        calls.append(cmd)
        if "--collect-only" in cmd:
            return subprocess.CompletedProcess(cmd, 0, "tests/test_x.py::test_0\ntests/test_x.py::test_1\n", "")
        raise subprocess.TimeoutExpired(cmd, kw["timeout"], output=b"partial output")

    monkeypatch.setattr(BC, "_dead", None)
    monkeypatch.setattr(BC, "_collected", {})
    monkeypatch.setattr(BC.subprocess, "run", run)
    with pytest.raises(AssertionError, match="collects 2 cases, at least 3 expected"):
        BC.run_bf16_child("tests/test_x.py", "x", 5, tmp_path, least=3)
    assert len(calls) == 1 and BC._dead is None, "too small a collection starts no child and is no death"
    with pytest.raises(AssertionError, match="no end after 5 s\npartial output"):
        BC.run_bf16_child("tests/test_x.py", "x", 5, tmp_path, least=2)
    assert len(calls) == 2 and "TimeoutExpired" in BC._dead
    with pytest.raises(AssertionError, match="not run: .* died with rc TimeoutExpired"):
        BC.run_bf16_child("tests/test_y.py", "y", 5, tmp_path, least=1)
    assert len(calls) == 2, "a process was started after a child had died"
