"""CPU: the batched DTU novel-view driver's pure parts — the reference's inference.yaml + overrides, the batch plan,
file names, resolutions, object tokens per mode and the decoder sub-batch choice."""
from types import SimpleNamespace

import pytest

from view_neti_amd import sd_config as sc
from view_neti_amd.compat import inference_dtu as nvs
from view_neti_amd.engine.infer import decode_sub_batch, decoder_sample_bytes

# input_configs/inference.yaml of the reference, verbatim
REFERENCE_YAML = """
input_dir: results/exp
iteration: 1500
seeds: [0,1]
torch_dtype: fp16
num_denoising_steps: 30
"""


def test_reference_inference_yaml_and_overrides(tmp_path):
    p = tmp_path / "inference.yaml"
    p.write_text(REFERENCE_YAML)
    c = nvs.parse_inference_config(["--config_path", str(p)])
    assert (c.iteration, str(c.input_dir), c.seeds, c.torch_dtype, c.num_denoising_steps) == \
        (1500, "results/exp", [0, 1], "fp16", 30)
    assert str(c.inference_dir) == "results/exp/inference" and c.batch == 8 and c.eval_placeholder_object_tokens == []
    c = nvs.parse_inference_config(["--config_path", str(p), "--input_dir", str(tmp_path / "run"), "--iteration", "2",
                                    "--seeds", "[3,4,5]", "--batch", "4", "--eval_placeholder_object_tokens",
                                    "[<scan114>]", "--num_denoising_steps", "2"])
    assert (c.iteration, c.seeds, c.batch, c.num_denoising_steps) == (2, [3, 4, 5], 4, 2)
    assert c.input_dir == tmp_path / "run" and c.inference_dir == tmp_path / "run" / "inference"
    assert c.eval_placeholder_object_tokens == ["<scan114>"]
    with pytest.raises(ValueError):
        nvs.parse_inference_config(["--config_path", str(p), "--torch_dtype", "fp32"])
    with pytest.raises(ValueError):
        nvs.parse_inference_config(["--config_path", str(p), "--no_such_key", "1"])


def test_batch_plan_order_and_padding():
    plan = nvs.plan_batches(["<a>", "<b>"], [1, 2, 3], [0, 1], 4)
    flat = [e for entries, n in plan for e in entries[:n]]
    assert flat == [(o, c, s) for o in ["<a>", "<b>"] for c in [1, 2, 3] for s in [0, 1]]
    assert [n for _, n in plan] == [4, 4, 4]
    plan = nvs.plan_batches([None], list(range(34)), [0, 1], 8)   # 68 views -> 8 full batches + 4 real entries
    assert len(plan) == 9 and all(len(e) == 8 for e, _ in plan) and plan[-1][1] == 4
    last, n = plan[-1]
    assert last[:n] == [(None, 32, 0), (None, 32, 1), (None, 33, 0), (None, 33, 1)] and last[n:] == [last[n - 1]] * 4
    assert nvs.plan_batches(["<a>"], [5], [7], 1) == [([("<a>", 5, 7)], 1)]


def test_reference_file_names():
    assert nvs.preds_png_name("<scan114>", 1500, 0) == "preds_object_<scan114>_iter_1500_seed0.png"
    assert nvs.preds_png_name(None, 2, 1) == "preds_object_None_iter_2_seed1.png"
    assert nvs.results_name(1500, [None], [0, 1]) == "results_all_iter_1500_scans_[None]_seeds_[0, 1].pt"
    assert nvs.results_name(3, ["<scan1>", "<scan2>"], [0]) == "results_all_iter_3_scans_['<scan1>', '<scan2>']_seeds_[0].pt"


def _cfg(mode, key=1, fixed="statue"):
    return SimpleNamespace(learnable_mode=mode, data=SimpleNamespace(dtu_preprocess_key=key,
                                                                     fixed_object_token_or_path=fixed))


def test_resolution_and_object_token_per_mode():
    assert nvs.nvs_resolution(_cfg(2, 1), sc.sd21()) == (576, 768)
    assert nvs.nvs_resolution(_cfg(2, 0), sc.sd21()) == (768, 768)
    assert nvs.nvs_resolution(_cfg(2, 0), sc.sd15()) == (512, 512)
    toks = ["<scan1>", "<scan2>"]
    assert nvs.eval_object_token(_cfg(1), []) == "statue"                # mode 1: the fixed word
    assert nvs.eval_object_token(_cfg(2), toks) == "<scan1>"             # modes 2/4/5: the learned token
    assert nvs.eval_object_token(_cfg(3), toks, "<scan2>") == "<scan2>"  # mode 3: the evaluation token
    with pytest.raises(ValueError):
        nvs.eval_object_token(_cfg(3), toks, "<scan9>")


def test_decoder_sub_batch():
    vae = sc.sd21().vae
    # 768 x 768: the 256-channel full-resolution level is 302 MB per sample, 2.4 GB at B = 8
    assert decoder_sample_bytes(vae, 96, 96) == 768 * 768 * 256 * 2
    assert decode_sub_batch(vae, 96, 96, 8) == 4 and decode_sub_batch(vae, 96, 96, 4) == 4
    assert decode_sub_batch(vae, 72, 96, 8) == 8          # 768 x 576 fits whole
    assert decode_sub_batch(vae, 96, 96, 7) == 7          # 2.11 GB: just inside the range
    assert decode_sub_batch(vae, 96, 96, 9) == 3          # the largest divisor under the limit
    assert decode_sub_batch(sc.sd15().vae, 64, 64, 8) == 8
