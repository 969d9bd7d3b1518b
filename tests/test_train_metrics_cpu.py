"""Host side of the per-step training record and of `optim.max_grad_norm`: configuration,
checkpoint contents, resume fingerprint, ring dump -> rows -> JSON lines, and the file's truncation on a resume.  No GPU."""
import json

import pytest
import torch

from view_neti_amd.compat import config as C
from view_neti_amd.compat import resume as R
from view_neti_amd.compat import train_metrics as TM
from view_neti_amd.engine import telemetry as T


# ------------------------------------------------------------------------------------------------ configuration
def test_fields_parse_and_validate():
    cfg = C.parse(C.RunConfig, ["--optim.max_grad_norm", "1.0", "--log.train_metrics", "true"])
    assert cfg.optim.max_grad_norm == 1.0 and isinstance(cfg.optim.max_grad_norm, float) and cfg.log.train_metrics is True
    plain = C.parse(C.RunConfig, [])
    assert plain.optim.max_grad_norm is None and plain.log.train_metrics is False
    for bad in ("0", "-1.0", "0.0"):
        with pytest.raises(ValueError, match="max_grad_norm"):
            C.parse(C.RunConfig, ["--optim.max_grad_norm", bad])
    # round trip through the YAML text of config.yaml
    again = C.decode(C.RunConfig, __import__("yaml").safe_load(C.dump(cfg)))
    assert again.optim.max_grad_norm == 1.0 and again.log.train_metrics is True


def test_what_a_checkpoint_and_config_yaml_carry():
    cfg = C.parse(C.RunConfig, ["--optim.max_grad_norm", "1.0", "--log.train_metrics", "true"])
    ckpt_cfg = C.encode(cfg, include_ext=False)
    assert "train_metrics" not in ckpt_cfg["log"] and "max_grad_norm" not in ckpt_cfg["optim"]
    C.decode(C.RunConfig, ckpt_cfg)  # still the reference's schema
    ext = C.ext_fields(cfg)
    assert ext["optim.max_grad_norm"] == 1.0 and not any("train_metrics" in k for k in ext)  # run control: never
    full = C.encode(cfg)
    assert full["optim"]["max_grad_norm"] == 1.0 and full["log"]["train_metrics"] is True
    # a run that uses neither writes the files it always wrote
    plain = C.parse(C.RunConfig, [])
    assert not any("max_grad_norm" in k or "train_metrics" in k for k in C.ext_fields(plain))
    assert "max_grad_norm" not in C.encode(plain)["optim"] and "train_metrics" not in C.encode(plain)["log"]


def test_fingerprint_has_the_field_only_when_set():
    args = (0, 2, 2, 1, "fp16", 0, 300, 1234)
    unset, clipped = R.fingerprint(*args), R.fingerprint(*args, max_grad_norm=1.0)
    assert "max_grad_norm" not in unset and clipped["max_grad_norm"] == 1.0
    assert {k: v for k, v in clipped.items() if k != "max_grad_norm"} == unset
    old = dict(unset)  # what a state saved before the field existed holds
    R.check_fingerprint(old, unset)
    R.check_fingerprint(clipped, clipped)
    for saved, current in ((old, clipped), (clipped, unset), (clipped, R.fingerprint(*args, max_grad_norm=2.0))):
        with pytest.raises(ValueError, match="max_grad_norm") as err:
            R.check_fingerprint(saved, current)
        assert "learnable_mode" not in str(err.value)


# ------------------------------------------------------------------------------------------------ ring -> rows
def _write(ring, c, batch, micro, t, losses, closed=None):
    """what the device writes for micro-step c (vneti_train_record, then vneti_grad_norm_finish when it closed a group)"""
    row = ring[c % ring.shape[0]]
    row.zero_()
    row[T.SEQ], row[T.MICRO] = c & T.SEQ_MASK, micro
    row[T.HEADER:T.HEADER + batch] = torch.tensor(t, dtype=torch.float32)
    row[T.HEADER + batch:] = torch.tensor(losses, dtype=torch.float32)
    if closed is not None:
        row[T.CLOSED] = 1.0
        for k, v in closed.items():
            row[k] = v


def _synthetic(accum=3, batch=2, steps=3, skipped_step=1, rows=32, no_object=False):
    ring = torch.zeros(rows, T.row_floats(batch))
    c, truth = 0, []
    for s in range(steps):
        samples = []
        for m in range(accum):
            t = [(37 * c + 11 * b) % 1000 for b in range(batch)]
            losses = [0.125 * (c + 1) + 0.5 * b for b in range(batch)]
            samples += list(zip(t, losses))
            closed = None
            if m == accum - 1:
                bad = s == skipped_step
                closed = {T.NORM_OBJECT: -1.0 if no_object else (float("inf") if bad else 3.0),
                          T.NORM_VIEW: float("nan") if bad else 4.0, T.NORM_TOTAL: float("inf") if bad else 5.0,
                          T.FINITE: 0.0 if bad else 1.0, T.CLIP_COEF: 1.0 if bad else 0.25,
                          T.LOSS_SCALE: 65536.0 * 0.5 ** (s > skipped_step), T.LR: 0.5 ** (s + 1)}
            _write(ring, c, batch, m, t, losses, closed)
            c += 1
        truth.append(samples)
    return ring, c, truth


def test_rows_to_json_lines():
    """a ring dump of grad_accum 3, B 2 with one skipped step -> the documented lines"""
    ring, count, truth = _synthetic()
    rows, lost = T.decode_ring(ring, count, 0, 2)
    assert lost == 0 and len(rows) == 9 and [r["micro"] for r in rows] == [0, 1, 2] * 3
    groups, open_rows, dropped = TM.group_rows(rows)
    assert len(groups) == 3 and not open_rows and dropped == 0
    lines = TM.lines_up_to(groups, 12)
    assert [l["step"] for l in lines] == [10, 11, 12]
    for l, samples in zip(lines, truth):
        assert list(l) == ["step", "loss", "lr", "loss_scale", "skipped", "grad_norm", "clip_coef", "samples"]
        assert len(l["samples"]) == 6 and l["samples"] == [{"t": t, "loss": x} for t, x in samples]
        assert l["loss"] == sum(x for _, x in samples) / 6  # (the values are exact in f32)
    ok, skipped, after = lines
    assert ok["skipped"] is False and ok["grad_norm"] == {"object": 3.0, "view": 4.0, "total": 5.0} and ok["clip_coef"] == 0.25
    assert ok["lr"] == 0.5 and ok["loss_scale"] == 65536.0
    assert skipped["skipped"] is True and skipped["clip_coef"] == 1.0
    assert skipped["grad_norm"] == {"object": None, "view": None, "total": None}  # JSON has no inf / nan
    assert after["loss_scale"] == 32768.0 and after["skipped"] is False and after["lr"] == 0.125
    for l in lines:
        assert json.loads(json.dumps(l, allow_nan=False)) == l
    # a side the device marks absent (-1) is omitted; Coach may also omit one it knows is a stand-in
    ring, count, _ = _synthetic(no_object=True)
    groups, _, _ = TM.group_rows(T.decode_ring(ring, count, 0, 2)[0])
    assert list(TM.step_line(1, groups[0])["grad_norm"]) == ["view", "total"]
    assert list(TM.step_line(1, groups[0], omit_view=True)["grad_norm"]) == ["total"]
    # rows since the last read only, and an accumulation group that is still open is handed back, not written
    ring, count, _ = _synthetic()
    rows, lost = T.decode_ring(ring, count - 1, 3, 2)
    assert lost == 0 and [r["micro_step"] for r in rows] == [3, 4, 5, 6, 7]
    groups, open_rows, dropped = TM.group_rows(rows)
    assert len(groups) == 1 and [r["micro_step"] for r in open_rows] == [6, 7] and dropped == 0


def test_lap_handling():
    """an 8-row ring read after 13 micro-steps: the 8 newest, oldest first, 5 reported lost; rows of another lap are never
    handed out as data"""
    batch, rows_n = 1, 8
    ring = torch.zeros(rows_n, T.row_floats(batch))
    for c in range(13):
        _write(ring, c, batch, 0, [c], [float(c)], closed={T.FINITE: 1.0, T.NORM_TOTAL: 1.0, T.CLIP_COEF: 1.0})
    rows, lost = T.decode_ring(ring, 13, 0, batch)
    assert lost == 5 and [r["micro_step"] for r in rows] == list(range(5, 13)) and [r["timesteps"] for r in rows] == [[c] for c in range(5, 13)]
    # 10 micro-steps since a read at 3: 8 are left, 2 are gone
    rows, lost = T.decode_ring(ring, 13, 3, batch)
    assert lost == 2 and [r["micro_step"] for r in rows] == list(range(5, 13))
    assert T.decode_ring(ring, 13, 13, batch) == ([], 0)
    # a dump whose counter is a lap ahead of its rows (rows 13, 14 not written yet): those two are lost, not read as 5, 6
    rows, lost = T.decode_ring(ring, 15, 9, batch)
    assert [r["micro_step"] for r in rows] == [9, 10, 11, 12] and lost == 2
    # a group whose first micro-step the ring has lost is dropped with its rows
    ring, count, _ = _synthetic(rows=7)
    rows, lost = T.decode_ring(ring, count, 0, 2)
    assert lost == 2 and [r["micro_step"] for r in rows] == [2, 3, 4, 5, 6, 7, 8]
    groups, open_rows, dropped = TM.group_rows(rows)
    assert dropped == 1 and len(groups) == 2 and [l["step"] for l in TM.lines_up_to(groups, 3)] == [2, 3]
    assert T.default_rows(50, 3) == 300


def test_file_truncates_on_resume(tmp_path):
    f = TM.TrainMetricsFile(tmp_path, 0)
    assert f.path == tmp_path / "train-metrics.jsonl" and f.path.read_text() == "" and f.last is None
    f.append([{"step": s, "loss": 0.5 * s} for s in range(1, 8)])
    assert f.last["step"] == 7
    text = f.path.read_text()
    with f.path.open("a") as h:
        h.write('{"step": 8, "lo')  # a write cut short
    g = TM.TrainMetricsFile(tmp_path, 5)  # resume from step 5
    assert g.kept == 5 and g.path.read_text() == "".join(text.splitlines(keepends=True)[:5])
    g.append([{"step": 6, "loss": 3.0}])
    assert [json.loads(l)["step"] for l in g.path.read_text().splitlines()] == [1, 2, 3, 4, 5, 6]
    assert not [p.name for p in tmp_path.iterdir() if p.name.endswith(".tmp")]
    assert TM.TrainMetricsFile(tmp_path, 0).path.read_text() == ""  # a fresh run starts the file empty
