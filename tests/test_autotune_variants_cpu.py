"""The autotuner's variant enumeration and pick serialisation, without a GPU.

`gemm_variants` decides what gets timed and so which kernels a run uses.  The expected lists below were recorded from the
autotuner BEFORE the enumeration was split out of its timing loop (its loop run with ops.gemm replaced by a recorder of
(tile_hint, split_k, conv korder), one entry per timed variant, in timing order); they are literals, not output of the
function under test.  Order matters: of equally fast variants the first one timed is pinned."""
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANDIDATES = (1, 2, 3, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18)  # Schedule.autotune's default


def _conv(mode, Hi, Ci, Ho, stride):
    return dict(mode=mode, Hi=Hi, Wi=Hi, Ci=Ci, Ho=Ho, Wo=Ho, stride=stride, pad_t=1, pad_l=1, ups=0, ldx=Ci, korder=0)


# name -> (key = Schedule._gemm_key's (M, N, K, batch, conv key, f32 out, geglu), conv dict, geglu)
PROBLEMS = {
    "deep_k_linear": ((308, 768, 3072, 1, None, False, 0), None, 0),  # small grid, deep K: explicit split factors
    "large_grid_linear": ((8192, 2560, 320, 1, None, False, 0), None, 0),  # >= 256 tiles at every tile size: (0, 1) only
    "geglu": ((2048, 2560, 320, 1, None, False, 1), None, 1),  # no GEGLU epilogue in the split-K reduce: split 1 only
    # stride-1 pad-1 3x3 on a 32 x 32 grid, B = 2: chunk-major for 16 / 17 and the halo tile 18
    "conv3x3_ci320": ((2048, 320, 2880, 1, (1, 1, 0, 32, 32), False, 0), _conv(1, 32, 320, 32, 1), 0),
    "conv3x3_ci64": ((2048, 64, 576, 1, (1, 1, 0, 32, 32), False, 0), _conv(1, 32, 64, 32, 1), 0),  # Ci < 128: no chunk-major
    # the split factors differ per tile size: >= 256 tiles at 64 x 64, the 16 Mi-float workspace caps the factor at 6
    "mixed_grid_linear": ((4096, 640, 5760, 1, None, False, 0), None, 0),
    "dgrad_stride2": ((2048, 320, 2880, 1, (2, 2, 0, 16, 16), False, 0), _conv(2, 16, 320, 32, 2), 0),  # no chunk-major
}

EXPECTED = {
    # key (308, 768, 3072, 1, None, False, 0)
    'deep_k_linear': [
        (1, 0, 0), (1, 1, 0), (1, 2, 0), (1, 3, 0), (1, 4, 0), (1, 6, 0), (2, 0, 0), (2, 1, 0), (2, 2, 0), (2, 3, 0),
        (2, 4, 0), (2, 6, 0), (3, 0, 0), (3, 1, 0), (3, 2, 0), (3, 3, 0), (3, 4, 0), (3, 6, 0), (5, 0, 0), (5, 1, 0),
        (5, 2, 0), (5, 3, 0), (5, 4, 0), (5, 6, 0), (6, 0, 0), (6, 1, 0), (6, 2, 0), (6, 3, 0), (6, 4, 0), (6, 6, 0),
        (7, 0, 0), (7, 1, 0), (7, 2, 0), (7, 3, 0), (7, 4, 0), (7, 6, 0), (8, 0, 0), (8, 1, 0), (8, 2, 0), (8, 3, 0),
        (8, 4, 0), (8, 6, 0), (9, 0, 0), (9, 1, 0), (9, 2, 0), (9, 3, 0), (9, 4, 0), (9, 6, 0), (10, 0, 0), (10, 1,
        0), (10, 2, 0), (10, 3, 0), (10, 4, 0), (10, 6, 0), (11, 0, 0), (11, 1, 0), (11, 2, 0), (11, 3, 0), (11, 4,
        0), (11, 6, 0), (12, 0, 0), (12, 1, 0), (12, 2, 0), (12, 3, 0), (12, 4, 0), (12, 6, 0), (13, 0, 0), (13, 1,
        0), (13, 2, 0), (13, 3, 0), (13, 4, 0), (13, 6, 0), (14, 0, 0), (14, 1, 0), (14, 2, 0), (14, 3, 0), (14, 4,
        0), (14, 6, 0), (15, 0, 0), (15, 1, 0), (15, 2, 0), (15, 3, 0), (15, 4, 0), (15, 6, 0), (16, 0, 0), (16, 1,
        0), (16, 2, 0), (16, 3, 0), (16, 4, 0), (16, 6, 0), (17, 0, 0), (17, 1, 0), (17, 2, 0), (17, 3, 0), (17, 4,
        0), (17, 6, 0)
    ],
    # key (8192, 2560, 320, 1, None, False, 0)
    'large_grid_linear': [
        (1, 0, 0), (1, 1, 0), (2, 0, 0), (2, 1, 0), (3, 0, 0), (3, 1, 0), (5, 0, 0), (5, 1, 0), (6, 0, 0), (6, 1, 0),
        (7, 0, 0), (7, 1, 0), (8, 0, 0), (8, 1, 0), (9, 0, 0), (9, 1, 0), (10, 0, 0), (10, 1, 0), (11, 0, 0), (11, 1,
        0), (12, 0, 0), (12, 1, 0), (13, 0, 0), (13, 1, 0), (14, 0, 0), (14, 1, 0), (15, 0, 0), (15, 1, 0), (16, 0,
        0), (16, 1, 0), (17, 0, 0), (17, 1, 0)
    ],
    # key (2048, 2560, 320, 1, None, False, 1)
    'geglu': [
        (1, 1, 0), (2, 1, 0), (3, 1, 0), (5, 1, 0), (6, 1, 0), (7, 1, 0), (8, 1, 0), (9, 1, 0), (10, 1, 0), (11, 1,
        0), (12, 1, 0), (13, 1, 0), (14, 1, 0), (15, 1, 0), (16, 1, 0), (17, 1, 0)
    ],
    # key (2048, 320, 2880, 1, (1, 1, 0, 32, 32), False, 0)
    'conv3x3_ci320': [
        (1, 0, 0), (1, 1, 0), (1, 2, 0), (1, 3, 0), (1, 4, 0), (2, 0, 0), (2, 1, 0), (2, 2, 0), (2, 3, 0), (2, 4, 0),
        (3, 0, 0), (3, 1, 0), (3, 2, 0), (3, 3, 0), (3, 4, 0), (5, 0, 0), (5, 1, 0), (5, 2, 0), (5, 3, 0), (5, 4, 0),
        (6, 0, 0), (6, 1, 0), (6, 2, 0), (6, 3, 0), (6, 4, 0), (7, 0, 0), (7, 1, 0), (7, 2, 0), (7, 3, 0), (7, 4, 0),
        (8, 0, 0), (8, 1, 0), (8, 2, 0), (8, 3, 0), (8, 4, 0), (9, 0, 0), (9, 1, 0), (9, 2, 0), (9, 3, 0), (9, 4, 0),
        (10, 0, 0), (10, 1, 0), (10, 2, 0), (10, 3, 0), (10, 4, 0), (11, 0, 0), (11, 1, 0), (11, 2, 0), (11, 3, 0),
        (11, 4, 0), (12, 0, 0), (12, 1, 0), (12, 2, 0), (12, 3, 0), (12, 4, 0), (13, 0, 0), (13, 1, 0), (13, 2, 0),
        (13, 3, 0), (13, 4, 0), (14, 0, 0), (14, 1, 0), (14, 2, 0), (14, 3, 0), (14, 4, 0), (15, 0, 0), (15, 1, 0),
        (15, 2, 0), (15, 3, 0), (15, 4, 0), (16, 0, 0), (16, 1, 0), (16, 2, 0), (16, 3, 0), (16, 4, 0), (17, 0, 0),
        (17, 1, 0), (17, 2, 0), (17, 3, 0), (17, 4, 0), (16, 0, 1), (16, 1, 1), (16, 2, 1), (16, 3, 1), (16, 4, 1),
        (17, 0, 1), (17, 1, 1), (17, 2, 1), (17, 3, 1), (17, 4, 1), (18, 0, 1), (18, 1, 1), (18, 2, 1), (18, 3, 1),
        (18, 4, 1)
    ],
    # key (2048, 64, 576, 1, (1, 1, 0, 32, 32), False, 0)
    'conv3x3_ci64': [
        (1, 0, 0), (1, 1, 0), (2, 0, 0), (2, 1, 0), (3, 0, 0), (3, 1, 0), (5, 0, 0), (5, 1, 0), (6, 0, 0), (6, 1, 0),
        (7, 0, 0), (7, 1, 0), (8, 0, 0), (8, 1, 0), (9, 0, 0), (9, 1, 0), (10, 0, 0), (10, 1, 0), (11, 0, 0), (11, 1,
        0), (12, 0, 0), (12, 1, 0), (13, 0, 0), (13, 1, 0), (14, 0, 0), (14, 1, 0), (15, 0, 0), (15, 1, 0), (16, 0,
        0), (16, 1, 0), (17, 0, 0), (17, 1, 0)
    ],
    # key (4096, 640, 5760, 1, None, False, 0)
    'mixed_grid_linear': [
        (1, 0, 0), (1, 1, 0), (1, 2, 0), (1, 3, 0), (1, 4, 0), (1, 6, 0), (2, 0, 0), (2, 1, 0), (3, 0, 0), (3, 1, 0),
        (5, 0, 0), (5, 1, 0), (5, 2, 0), (5, 3, 0), (5, 4, 0), (5, 6, 0), (6, 0, 0), (6, 1, 0), (6, 2, 0), (6, 3, 0),
        (6, 4, 0), (6, 6, 0), (7, 0, 0), (7, 1, 0), (7, 2, 0), (7, 3, 0), (7, 4, 0), (7, 6, 0), (8, 0, 0), (8, 1, 0),
        (8, 2, 0), (8, 3, 0), (8, 4, 0), (8, 6, 0), (9, 0, 0), (9, 1, 0), (9, 2, 0), (9, 3, 0), (9, 4, 0), (9, 6, 0),
        (10, 0, 0), (10, 1, 0), (10, 2, 0), (10, 3, 0), (10, 4, 0), (10, 6, 0), (11, 0, 0), (11, 1, 0), (12, 0, 0),
        (12, 1, 0), (13, 0, 0), (13, 1, 0), (13, 2, 0), (13, 3, 0), (13, 4, 0), (13, 6, 0), (14, 0, 0), (14, 1, 0),
        (15, 0, 0), (15, 1, 0), (16, 0, 0), (16, 1, 0), (16, 2, 0), (16, 3, 0), (16, 4, 0), (16, 6, 0), (17, 0, 0),
        (17, 1, 0), (17, 2, 0), (17, 3, 0), (17, 4, 0), (17, 6, 0)
    ],
    # key (2048, 320, 2880, 1, (2, 2, 0, 16, 16), False, 0)
    'dgrad_stride2': [
        (1, 0, 0), (1, 1, 0), (1, 2, 0), (1, 3, 0), (1, 4, 0), (2, 0, 0), (2, 1, 0), (2, 2, 0), (2, 3, 0), (2, 4, 0),
        (3, 0, 0), (3, 1, 0), (3, 2, 0), (3, 3, 0), (3, 4, 0), (5, 0, 0), (5, 1, 0), (5, 2, 0), (5, 3, 0), (5, 4, 0),
        (6, 0, 0), (6, 1, 0), (6, 2, 0), (6, 3, 0), (6, 4, 0), (7, 0, 0), (7, 1, 0), (7, 2, 0), (7, 3, 0), (7, 4, 0),
        (8, 0, 0), (8, 1, 0), (8, 2, 0), (8, 3, 0), (8, 4, 0), (9, 0, 0), (9, 1, 0), (9, 2, 0), (9, 3, 0), (9, 4, 0),
        (10, 0, 0), (10, 1, 0), (10, 2, 0), (10, 3, 0), (10, 4, 0), (11, 0, 0), (11, 1, 0), (11, 2, 0), (11, 3, 0),
        (11, 4, 0), (12, 0, 0), (12, 1, 0), (12, 2, 0), (12, 3, 0), (12, 4, 0), (13, 0, 0), (13, 1, 0), (13, 2, 0),
        (13, 3, 0), (13, 4, 0), (14, 0, 0), (14, 1, 0), (14, 2, 0), (14, 3, 0), (14, 4, 0), (15, 0, 0), (15, 1, 0),
        (15, 2, 0), (15, 3, 0), (15, 4, 0), (16, 0, 0), (16, 1, 0), (16, 2, 0), (16, 3, 0), (16, 4, 0), (17, 0, 0),
        (17, 1, 0), (17, 2, 0), (17, 3, 0), (17, 4, 0)
    ],
}


@pytest.mark.parametrize("name", list(PROBLEMS))
def test_variants_are_those_the_autotuner_timed(name):
    from view_neti_amd.engine.schedule import gemm_variants
    key, conv, geglu = PROBLEMS[name]
    before = json.dumps(conv)
    got = gemm_variants(key, conv, geglu, CANDIDATES)
    assert got == EXPECTED[name]
    assert json.dumps(conv) == before, "the conv dict is the launch's own: not to be modified"


def test_expected_lists_show_the_rules():
    """what each problem is in the list for (a check of the literals themselves)"""
    E = EXPECTED
    splits = lambda name, tile, ko=0: [s for t, s, k in E[name] if t == tile and k == ko]
    assert splits("deep_k_linear", 1) == [0, 1, 2, 3, 4, 6]
    assert {s for _, s, _ in E["large_grid_linear"]} == {0, 1}
    assert {s for _, s, _ in E["geglu"]} == {1} and len(E["geglu"]) == 16
    assert {t for t, _, k in E["conv3x3_ci320"] if k == 1} == {16, 17, 18}
    assert all(k == 1 for t, _, k in E["conv3x3_ci320"] if t == 18)  # the halo tile runs chunk-major only
    assert E["conv3x3_ci320"].index((17, 4, 0)) < E["conv3x3_ci320"].index((16, 0, 1))  # tap-major first
    for name in ("conv3x3_ci64", "dgrad_stride2", "deep_k_linear"):
        assert all(k == 0 and t != 18 for t, _, k in E[name])
    assert splits("mixed_grid_linear", 3) == [0, 1] and splits("mixed_grid_linear", 1) == [0, 1, 2, 3, 4, 6]


def test_candidates_restrict_the_variants():
    from view_neti_amd.engine.schedule import gemm_variants
    key, conv, geglu = PROBLEMS["conv3x3_ci320"]
    assert gemm_variants(key, conv, geglu, (17, 18)) == [v for v in EXPECTED["conv3x3_ci320"] if v[0] in (17, 18)]
    assert gemm_variants(key, dict(conv, Ho=24, Wo=24, Hi=24, Wi=24), geglu, (18,)) == []  # no 16-pixel grid: no halo tile


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_pick_serialisation_round_trips_the_committed_picks(precision):
    from view_neti_amd.engine.schedule import picks_from_json, picks_to_json
    with open(os.path.join(ROOT, "bench_picks.json")) as fh:
        on_disk = json.load(fh)[precision]
    assert len(on_disk) > 50
    cache = picks_from_json(on_disk)
    assert len(cache) == len(on_disk)
    for key, pick in cache.items():
        assert isinstance(key, tuple) and len(key) == 7 and isinstance(pick, tuple) and len(pick) in (2, 3)
        assert all(type(x) is int for x in pick)
    back = picks_to_json(cache)
    assert list(back) == list(on_disk)  # key for key, in the file's order
    for k in on_disk:
        assert back[k] == on_disk[k], k


def test_preload_picks_refuses_a_foreign_kernel_tree():
    from view_neti_amd.engine import schedule as S
    from view_neti_amd.roofline import kernel_tree_sha
    saved = dict(S.Schedule._tile_cache)
    S.Schedule._tile_cache.clear()
    try:
        picks = {repr((308, 768, 3072, 1, None, False, 0)): [17, 2, 0], repr((64, 64, 64, 1, None, True, 0)): [3, 1]}
        assert S.preload_picks({"kernel_tree_sha": "0" * 16, "picks": picks}) is False
        assert S.preload_picks({"picks": picks}) is False
        assert S.Schedule._tile_cache == {}, "refused picks must not be loaded, not even in part"
        assert S.preload_picks({"kernel_tree_sha": kernel_tree_sha(), "picks": picks}) is True
        assert S.Schedule._tile_cache == {(308, 768, 3072, 1, None, False, 0): (17, 2, 0),
                                          (64, 64, 64, 1, None, True, 0): (3, 1)}
        assert S.export_picks() == {"kernel_tree_sha": kernel_tree_sha(), "picks": picks}
    finally:
        S.Schedule._tile_cache.clear()
        S.Schedule._tile_cache.update(saved)
