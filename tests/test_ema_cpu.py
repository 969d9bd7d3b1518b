"""The exponential moving average of the mappers without a GPU: the float64 restatement of the
decay and the update (tests/helpers/ema_ref.py), the configuration fields and where they travel, the names of the averaged
checkpoints and their selection by `--use_ema`, and the held-out record with and without the average."""
import json
from types import SimpleNamespace

import numpy as np
import pytest

from helpers import ema_ref as ER
from view_neti_amd.compat import config as C
from view_neti_amd.compat import heldout as H
from view_neti_amd.compat import inference_dtu as NVS
from view_neti_amd.compat import resume as R


# ------------------------------------------------------------------------------------------------ the recurrence
def test_decay_values():
    assert ER.decay(1, 0.9999) == 0.0                                    # k = 1: s = 0, the first update is a copy
    assert ER.decay(2, 0.9999) == 2.0 / 11.0                             # s = 1
    assert ER.decay(9, 0.9999) == 0.5 and ER.decay(8, 0.5) == 8.0 / 17.0  # the ramp reaches 0.5 at s = 8 ...
    assert all(ER.decay(k, 0.5) == 0.5 for k in range(9, 200))           # ... and max_decay = 0.5 caps from there
    assert ER.decay(10, 0.9999) == 10.0 / 19.0 > 0.5
    assert ER.decay(2, 0.9999, power=2.0 / 3.0) == 1.0 - 2.0 ** (-2.0 / 3.0)
    assert [ER.decay(k, 0.9999, 3) for k in range(1, 5)] == [0.0] * 4    # update_after_step = 3: 0 through k = 4
    assert ER.decay(5, 0.9999, 3) == 2.0 / 11.0
    assert ER.decay(10 ** 9, 0.9999) == 0.9999 and ER.decay(10 ** 9, 0.9999, power=0.75) == 0.9999
    ramp = [ER.decay(k, 0.9999) for k in range(1, 400)]
    assert all(a < b for a, b in zip(ramp, ramp[1:]))


def _run(ps, max_decay, after=0, power=0.0):
    """the engine's recurrence on a sequence of parameter vectors: ema starts as a clone of the first"""
    e, out = np.array(ps[0], dtype=np.float64), []
    for k, p in enumerate(ps, 1):
        d = ER.decay(k, max_decay, after, power)
        e = np.array(p, dtype=np.float64) if d == 0.0 else ER.update(e, p, 1.0 - d)
        out.append(e)
    return out


def test_constant_parameters_stay_put():
    p = np.array([1.5, -0.25, 3e-7, 0.0])
    for power in (0.0, 2.0 / 3.0):
        for e in _run([p] * 50, 0.999, power=power):
            assert np.array_equal(e, p)  # p - e is exactly 0: the update changes no bit


def test_a_step_in_p_is_approached_geometrically():
    """p steps once, from a to b, after the average equals a; from then on the distance to b shrinks by d per update"""
    a, b, d = np.array([1.0, -2.0]), np.array([3.0, 5.0]), 0.5
    es = _run([a] * 20 + [b] * 12, d)  # k >= 9: the decay is the cap 0.5
    assert np.array_equal(es[19], a)
    dist = [np.abs(e - b) for e in es[19:]]
    for j in range(1, len(dist)):
        assert np.allclose(dist[j], d * dist[j - 1], rtol=1e-14, atol=0)
    assert np.allclose(dist[12], 0.5 ** 12 * np.abs(a - b), rtol=1e-13, atol=0)


# ------------------------------------------------------------------------------------------------ configuration
ON = ["--optim.ema_decay", "0.999", "--optim.ema_update_after_step", "10", "--optim.ema_warmup_power", "0.75"]
FIELDS = ("ema_decay", "ema_update_after_step", "ema_warmup_power")


def test_fields_parse_and_validate():
    cfg = C.parse(C.RunConfig, ON)
    o = cfg.optim
    assert (o.ema_decay, o.ema_update_after_step, o.ema_warmup_power) == (0.999, 10, 0.75)
    assert isinstance(o.ema_update_after_step, int)
    plain = C.parse(C.RunConfig, [])
    assert (plain.optim.ema_decay, plain.optim.ema_update_after_step, plain.optim.ema_warmup_power) == (None, 0, None)
    assert plain.eval.validation_use_ema is False
    for bad in ("0", "1", "1.5", "-0.1", "nan"):
        with pytest.raises(ValueError, match="ema_decay"):
            C.parse(C.RunConfig, ["--optim.ema_decay", bad])
    for bad in ("0", "-1", "inf", "nan"):
        with pytest.raises(ValueError, match="ema_warmup_power"):
            C.parse(C.RunConfig, ["--optim.ema_decay", "0.9", "--optim.ema_warmup_power", bad])
    with pytest.raises(ValueError, match="ema_update_after_step"):
        C.parse(C.RunConfig, ["--optim.ema_decay", "0.9", "--optim.ema_update_after_step", "-1"])
    for alone in (["--optim.ema_update_after_step", "3"], ["--optim.ema_warmup_power", "0.5"]):
        with pytest.raises(ValueError, match="ema_decay"):
            C.parse(C.RunConfig, alone)
    for again in (C.decode(C.RunConfig, C.encode(cfg)), C.decode(C.RunConfig, __import__("yaml").safe_load(C.dump(cfg)))):
        assert (again.optim.ema_decay, again.optim.ema_update_after_step, again.optim.ema_warmup_power) == (0.999, 10, 0.75)


def test_what_a_checkpoint_and_config_yaml_carry():
    cfg = C.parse(C.RunConfig, ON + ["--eval.validation_use_ema", "true"])
    ckpt_cfg = C.encode(cfg, include_ext=False)
    assert not any(f in ckpt_cfg["optim"] for f in FIELDS) and "validation_use_ema" not in ckpt_cfg["eval"]
    C.decode(C.RunConfig, ckpt_cfg)  # still the reference's schema
    ext = C.ext_fields(cfg)
    assert (ext["optim.ema_decay"], ext["optim.ema_update_after_step"], ext["optim.ema_warmup_power"]) == (0.999, 10, 0.75)
    assert not any("validation_use_ema" in k for k in ext)  # run control: never in a checkpoint
    full = C.encode(cfg)
    assert full["optim"]["ema_decay"] == 0.999 and full["eval"]["validation_use_ema"] is True
    only = C.parse(C.RunConfig, ["--optim.ema_decay", "0.9"])
    assert C.ext_fields(only)["optim.ema_decay"] == 0.9
    assert not any(k in C.ext_fields(only) for k in ("optim.ema_update_after_step", "optim.ema_warmup_power"))
    assert "ema_update_after_step" not in C.encode(only)["optim"] and "ema_warmup_power" not in C.encode(only)["optim"]
    plain = C.parse(C.RunConfig, [])
    assert not any("ema" in k for k in C.ext_fields(plain))
    assert not any("ema" in k for k in C.encode(plain)["optim"]) and not any("ema" in k for k in C.encode(plain)["eval"])


@pytest.mark.parametrize("field,value,other", [("ema_decay", 0.999, 0.99), ("ema_update_after_step", 10, 11),
                                               ("ema_warmup_power", 0.75, 0.5)])
def test_fingerprint_has_the_field_only_when_set(field, value, other):
    args = (0, 2, 2, 1, "fp16", 0, 300, 1234)
    unset, on = R.fingerprint(*args), R.fingerprint(*args, **{field: value})
    assert field not in unset and on[field] == value
    assert {k: v for k, v in on.items() if k != field} == unset
    assert R.fingerprint(*args, ema_decay=None, ema_update_after_step=0, ema_warmup_power=None) == unset
    R.check_fingerprint(dict(unset), unset)  # a state saved before the field existed
    R.check_fingerprint(on, on)
    for saved, current in ((unset, on), (on, unset), (on, R.fingerprint(*args, **{field: other}))):
        with pytest.raises(ValueError, match=field) as err:
            R.check_fingerprint(saved, current)
        assert "learnable_mode" not in str(err.value)


def test_engine_state_description_names_the_field():
    """the rule load_state_dict applies (engine/step.py), on the description alone: no GPU"""
    from view_neti_amd.engine.step import TrainStepEngine as E
    assert set(FIELDS) <= set(E._WHEN_SET) and "ema" not in E._STATE and "ema_count" not in E._STATE


# ------------------------------------------------------------------------------------------------ files
def test_ema_file_names(tmp_path):
    assert R.ema_name("mapper-steps-1500.pt") == "mapper-ema-steps-1500.pt"
    assert R.ema_name("mapper-final.pt") == "mapper-ema-final.pt"
    assert R.ema_name("mapper-steps-3_object.pt") == "mapper-ema-steps-3_object.pt"
    for bad in ("mapper-ema-steps-3.pt", "learned_embeds-final.bin"):
        with pytest.raises(ValueError):
            R.ema_name(bad)
    assert {k: f.name for k, f in R.ema_mapper_files(tmp_path, 7, 2).items()} == \
        {"object": "mapper-ema-steps-7_object.pt", "view": "mapper-ema-steps-7_view.pt"}
    assert list(R.ema_mapper_files(tmp_path, 7, 0)) == ["object"] and list(R.ema_mapper_files(tmp_path, 7, 1)) == ["view"]
    assert list(R.ema_mapper_files(tmp_path, 7, 4)) == ["object"]  # the frozen view mapper has no average
    # an averaged checkpoint is no step checkpoint: nothing resumes from it, and a state's completeness ignores it
    with pytest.raises(ValueError):
        R.parse_step("mapper-ema-steps-7_object.pt")
    assert not any("ema" in f.name for f in R.resume_files(tmp_path, 7, 2))


def test_use_ema_selects_the_averaged_files_or_raises(tmp_path):
    touch = lambda name: (tmp_path / name).write_bytes(b"")
    for name in ("mapper-steps-5_object.pt", "mapper-steps-5_view.pt"):
        touch(name)
    assert NVS.nvs_mapper_stems(tmp_path, 5, 2) == ("mapper-steps-5", "mapper-steps-5")
    with pytest.raises(FileNotFoundError, match="mapper-ema-steps-5_object.pt"):
        NVS.nvs_mapper_stems(tmp_path, 5, 2, use_ema=True)  # never the raw files in their place
    touch("mapper-ema-steps-5_object.pt")
    with pytest.raises(FileNotFoundError, match="mapper-ema-steps-5_view.pt") as err:
        NVS.nvs_mapper_stems(tmp_path, 5, 2, use_ema=True)
    assert "mapper-ema-steps-5_object.pt" not in str(err.value)
    assert NVS.nvs_mapper_stems(tmp_path, 5, 4, use_ema=True) == ("mapper-ema-steps-5", "mapper-steps-5")  # frozen view
    touch("mapper-ema-steps-5_view.pt")
    assert NVS.nvs_mapper_stems(tmp_path, 5, 2, use_ema=True) == ("mapper-ema-steps-5", "mapper-ema-steps-5")
    assert NVS.nvs_mapper_stems(tmp_path, 5, 1, use_ema=True) == ("mapper-steps-5", "mapper-ema-steps-5")
    icfg = C.parse(NVS.InferenceConfig, ["--input_dir", str(tmp_path), "--iteration", "5", "--use_ema", "true"])
    assert icfg.use_ema is True and C.parse(NVS.InferenceConfig, []).use_ema is False


# ------------------------------------------------------------------------------------------------ the held-out record
class _Ctx:
    def __init__(self, eng):
        self.eng = eng

    def __enter__(self):
        self.eng.swapped = True

    def __exit__(self, *a):
        self.eng.swapped = False


class _Engine:
    """what HeldoutLoss.run touches of the engine"""
    def __init__(self, ema):
        self.ema, self.swapped, self.entered = ema, False, 0

    def ema_weights(self):
        self.entered += 1
        return _Ctx(self)


def _evaluator(tmp_path, ema):
    p = H.plan(2, "dtu-12d", 3, ["<obj>"], 2, 4)
    ev = object.__new__(H.HeldoutLoss)
    eng = _Engine(ema)
    ev.coach = SimpleNamespace(engine=eng, cfg=SimpleNamespace(log=SimpleNamespace(exp_dir=tmp_path)), log=lambda msg: None)
    ev.plan = p

    def evaluate():  # a loss per item that says which weights the engine held
        return {obj: [(it, (0.5 if eng.swapped else 1.0) + 1e-3 * it.cam + it.k) for items, n in batches for it in items[:n]]
                for obj, batches in p.batches.items()}
    ev.evaluate = evaluate
    return ev, eng, p


def test_heldout_record_gains_ema_only_when_set(tmp_path):
    (tmp_path / "off").mkdir()
    (tmp_path / "on").mkdir()
    off, eng_off, p = _evaluator(tmp_path / "off", None)
    rec_off = off.run(3)
    assert eng_off.entered == 0 and "ema" not in rec_off["objects"]["<obj>"]
    # byte-identical to the line the code wrote before the average existed: make_record of the raw losses, dumped
    want = json.dumps(H.make_record(3, p, off.evaluate())) + "\n"
    assert (tmp_path / "off" / H.FILE_NAME).read_text() == want
    assert list(rec_off["objects"]["<obj>"]) == ["train", "test", "by_timestep", "by_view"]
    on, eng_on, _ = _evaluator(tmp_path / "on", object())
    rec_on = on.run(3)
    o = rec_on["objects"]["<obj>"]
    assert eng_on.entered == 1 and not eng_on.swapped
    assert list(o) == ["train", "test", "by_timestep", "by_view", "ema"]
    assert list(o["ema"]) == ["train", "test", "by_timestep", "by_view"]
    assert {k: v for k, v in o.items() if k != "ema"} == rec_off["objects"]["<obj>"]  # the raw fields are unchanged
    assert o["ema"]["train"] == pytest.approx(o["train"] - 0.5) and o["ema"]["test"] == pytest.approx(o["test"] - 0.5)
    (back,) = H.read_records(tmp_path / "on" / H.FILE_NAME)
    assert back["objects"]["<obj>"]["ema"]["by_view"] == {int(c): v for c, v in o["ema"]["by_view"].items()}
    assert "ema:" in H.summary_line(3, rec_on) and "ema" not in H.summary_line(3, rec_off)
