"""N > 1 on the HIP path (training/coach.py:728-733): two ranks share cuda:0 over the gloo backend and
run the CAPTURED TrainStepEngine(world_size=2) — graph A (forward + backward), the all-reduce(sum) of the flat
gradient bucket, graph B (AdamW with grad_div = world).  The ranks must end bit-identical, and must equal ONE
process that feeds the same two micro-batches through gradient accumulation (mean of two micro-gradients: the same
arithmetic).  Repeated for learnable_mode 3: three object mappers + the view mapper, the scene changing between
steps, where only the active scene's segment and the view mapper cross the wire (BASELINE config 4's DP leg)."""
import os

import pytest
import torch
import torch.multiprocessing as mp

from helpers.engines import STATES_FIRST, build_train_engine, feed_host_noise

pytestmark = pytest.mark.gpu

STEPS, B, H, W, LR = 3, 2, 64, 64, 3e-3
GRAD_TOL = 5e-3  # of max|g|, see below
SCENES = [0, 2, 0]


def _build(world, accum, mode3):
    # identical mapper initialisation on every rank: the reference gets it from the torch.manual_seed(0) inside every
    # FourierPositionalEncodingNDims constructor (App. C Q1); init_mapper_state draws from the global generator
    cfg, eng, _, _, _, _ = build_train_engine("tiny", B, H, W, n_obj=3 if mode3 else 1, with_view=mode3, perturb_seed=7,
                                              order=STATES_FIRST, lr=LR, world_size=world, grad_accum=accum, device_rng=False)
    return cfg, eng


def _feed(cfg, eng, step, shard, mode3):
    feed_host_noise(cfg, eng, step, shard, mode3, SCENES)


def _worker(rank, world, port, mode3, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      HSA_ENABLE_IPC_MODE_LEGACY="0", VNETI_NO_GN_FUSE="1")
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    cfg, eng = _build(world, 1, mode3)
    _feed(cfg, eng, 0, rank, mode3)
    eng.capture()
    assert eng.graph_b is not None, "world_size > 1 must split the step around the all-reduce"
    p0 = eng.params.clone()
    # every rank replays ONE schedule: rank 0 autotuned, the others took its picks (engine/schedule.py::autotune)
    from view_neti_amd import ops, parallel
    picks = [(f.keywords.get("tile_hint"), f.keywords.get("split_k"), (f.keywords.get("conv") or {}).get("korder"))
             for f in eng.launches() if getattr(f, "func", None) is ops.gemm]
    all_picks = [None] * world
    dist.all_gather_object(all_picks, picks)
    assert len(picks) > 50 and all(p == all_picks[0] for p in all_picks), "ranks pinned different GEMM tiles / split-K factors"
    losses, reduced, calls = [], [], []
    for step in range(STEPS):
        _feed(cfg, eng, step, rank, mode3)
        # == eng.step(), spelled out so the all-reduced gradient bucket can be looked at before AdamW clears it
        eng.graph_a.replay()
        c0 = parallel.COLLECTIVE_CALLS
        eng.all_reduce()
        calls.append(parallel.COLLECTIVE_CALLS - c0)
        reduced.append(eng.grads.cpu().clone())
        eng.graph_b.replay()
        losses.append(eng.loss())
    torch.cuda.synchronize()
    mine = eng.params.cpu()
    gathered = [torch.zeros_like(mine) for _ in range(world)]
    dist.all_gather(gathered, mine)
    if rank == 0:
        torch.save({"all": gathered, "p0": p0.cpu(), "losses": losses, "opt_step": int(eng.opt_step.item()),
                    "reduced": reduced, "scale": float(eng.scaler[0]), "calls": calls, "moved": eng.last_reduce_bytes,
                    "n_obj": eng.n_obj, "n_view": eng.grads.numel() - eng.n_all_obj,
                    "seg_step": eng.seg_step.cpu().tolist(), "grad_div": float(eng.hyper[5])}, out)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(900)
@pytest.mark.parametrize("mode3", [False, True], ids=["mode0", "mode3"])
def test_two_ranks_on_the_hip_engine_equal_grad_accumulation(tmp_path, mode3, monkeypatch):
    out = str(tmp_path / "dp.pt")
    port = 29600 + (os.getpid() % 300) + (50 if mode3 else 0)
    mp.spawn(_worker, args=(2, port, mode3, out), nprocs=2, join=True)
    res = torch.load(out)
    a, b = res["all"]
    assert torch.equal(a, b), "the two ranks' parameters must be bit-identical after the all-reduced steps"
    assert res["opt_step"] == STEPS and res["grad_div"] == 2.0 and all(l == l and l > 0 for l in res["losses"])
    # ONE collective per optimisation step (north_star), also in mode 3 where the active scene's segment and the view
    # mapper are packed into one contiguous buffer; the payload is exactly those two segments
    assert res["calls"] == [1] * STEPS
    assert res["moved"] == 4 * (res["n_obj"] + (res["n_view"] if mode3 else 0))
    # ---- one process, the same two micro-batches per step through gradient accumulation ----
    monkeypatch.setenv("VNETI_NO_GN_FUSE", "1")  # same (atomics-free, deterministic) schedule as the workers
    cfg, eng = _build(1, 2, mode3)
    _feed(cfg, eng, 0, 0, mode3)
    eng.capture()
    assert torch.equal(eng.params.cpu(), res["p0"])
    worst_g = 0.0
    for step in range(STEPS):
        _feed(cfg, eng, step, 0, mode3)
        assert eng.step() is False
        g0 = eng.grads.cpu().clone()
        _feed(cfg, eng, step, 1, mode3)
        eng.graph_acc.replay()                      # == the second micro-step of eng.step() up to the optimizer
        g01 = eng.grads.cpu().clone()
        # the accumulated bucket is the sum of the two micro-gradients ...
        eng.forward_backward(accumulate=False)      # micro-batch 1 alone (eager, same launches)
        torch.cuda.synchronize()
        g1 = eng.grads.cpu().clone()
        eng.grads.copy_(g01)
        # only the gradients this step owns: the active scene's segment and the view mapper (the other segments hold
        # whatever their last training step left — AdamW ignores them, DESIGN D10 — and are not all-reduced either)
        live = torch.zeros_like(g0, dtype=torch.bool)
        k = SCENES[step] if mode3 else 0
        live[k * eng.n_obj:(k + 1) * eng.n_obj] = True
        live[eng.n_all_obj:] = True
        ref_sum = (g0 + g1)[live]
        scale = max(ref_sum.abs().max().item(), 1e-30)
        # (tolerance: two runs of the SAME micro-batch differ by ~7e-4 of max|g| — the GroupNorm statistics are summed with
        #  LDS float atomics in varying order and the f16 roundings downstream amplify the last bit; from the second step
        #  on the two runs' parameters differ in the sign-flip entries described below, hence the looser bound there;
        #  a wrong divisor or a missing rank would be off by O(1))
        assert (g01[live] - ref_sum).abs().max().item() <= 5 * GRAD_TOL * scale
        # ... and so is what the two ranks all-reduced; both are divided by hyper[5] = 2 inside AdamW.  Step 0 starts from
        # identical parameters and is compared element-wise; afterwards the two runs' parameters differ in the sign-flip
        # entries described below (and their tile picks may differ: the workers autotune in fresh processes), so the later
        # steps are compared by direction and length
        red = res["reduced"][step][live]
        dg = (red - g01[live]).abs().max().item() / scale
        cos = torch.nn.functional.cosine_similarity(red, g01[live], dim=0).item()
        ratio = (red.norm() / g01[live].norm()).item()
        worst_g = max(worst_g, dg)
        if step == 0:
            assert dg <= GRAD_TOL, f"all-reduced gradients differ from the accumulated ones by {dg:.2e} of max|g|"
        assert cos > 0.98 and 0.9 < ratio < 1.1, f"step {step}: all-reduced vs accumulated gradients cos {cos:.4f} ratio {ratio:.3f}"
        eng.micro = 0
        eng.graph_b.replay()
    torch.cuda.synchronize()
    assert float(eng.hyper[5]) == 2.0 and float(eng.scaler[0]) == res["scale"]
    ref = eng.params.cpu()
    upd = (ref - res["p0"]).abs().max().item()
    dev = (a - ref).abs()
    # AdamW's first steps move every weight by ~lr * sign(g): entries whose gradient is ~0 may flip sign on the last
    # bit of the sums above, so the parameters are compared robustly (the gradients were compared exactly)
    frac_off = (dev > 0.05 * LR).float().mean().item()
    print(f"[dp gpu {'mode3' if mode3 else 'mode0'}] max |update| {upd:.3e}; all-reduced vs accumulated gradients: worst "
          f"{worst_g:.2e} of max|g|; params: median dev {dev.median().item():.2e}, {100 * frac_off:.3f}% of entries off by "
          f"> 0.05 lr; seg_step {res['seg_step']}")
    assert upd > 0.5 * LR, "three AdamW steps move the weights by ~lr each"
    assert dev.median().item() <= 0.02 * LR and frac_off < 0.05
    if mode3:
        n = eng.n_obj
        assert torch.equal(a[n:2 * n], res["p0"][n:2 * n]), "the scene that never trained must not move"
        # torch.optim.AdamW semantics (DESIGN D10): a mapper joins the update set when first trained and is stepped on
        # every iteration afterwards — scene 0 from step 1, scene 2 from step 2, scene 1 never
        assert res["seg_step"] == [3, 0, 2] and eng.seg_step.cpu().tolist() == [3, 0, 2]


def _coach_worker(rank, world, port, root, out_dir):
    """two ranks of the reference-shaped Coach with validation ENABLED (the default): rank 0 alone builds the validator's
    inference engines, whose autotuner must not issue collectives the other rank never joins"""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK="0", HSA_ENABLE_IPC_MODE_LEGACY="0")
    import datetime

    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=240))
    from view_neti_amd import parallel
    from view_neti_amd.compat import config as C
    from view_neti_amd.compat.coach import Coach
    cfg = C.parse(C.RunConfig, [
        "--data.train_data_dir", root, "--data.placeholder_object_token", "<toy>", "--data.resolution", "64",
        "--data.dataloader_num_workers", "0", "--model.word_embedding_dim", "128", "--model.arch_view_net", "15",
        "--model.arch_view_disable_tl", "False", "--model.arch_mlp_hidden_dims", "64", "--model.use_nested_dropout",
        "False", "--optim.max_train_steps", "4", "--optim.train_batch_size", "2",
        "--optim.gradient_accumulation_steps", "1", "--optim.mixed_precision", "fp16", "--log.save_steps", "4",
        "--eval.validation_steps", "2", "--eval.num_denoising_steps", "2", "--eval.num_validation_images", "1",
        "--eval.validation_seeds", "[0]", "--log.exp_dir", out_dir, "--log.exp_name", "dp"])
    cfg.log.exp_dir = cfg.log.exp_dir / cfg.log.exp_name
    cfg.log.logging_dir = cfg.log.exp_dir / cfg.log.logging_dir
    torch.manual_seed(cfg.seed)
    coach = Coach(cfg)
    assert (coach.validator is not None) == (rank == 0)
    c0 = parallel.COLLECTIVE_CALLS
    coach.train()
    torch.cuda.synchronize()
    # 4 optimisation steps + the warm-up step inside capture() (a real, all-reduced step whose state is rolled back)
    assert parallel.COLLECTIVE_CALLS - c0 == 5, "one gradient all-reduce per optimisation step, nothing else on the data path"
    mine = coach.engine.params.cpu()
    both = [torch.zeros_like(mine) for _ in range(world)]
    dist.all_gather(both, mine)
    assert torch.equal(both[0], both[1]), "ranks diverged: a collective was mis-paired"
    assert int(coach.engine.opt_step.item()) == 4 and abs(float(coach.engine.hyper[0]) - 1e-3 * 2 * 2) < 1e-9
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(900)
def test_two_rank_coach_with_rank0_only_validator(tmp_path):
    import numpy as np
    from PIL import Image
    root = tmp_path / "toys"
    root.mkdir()
    rng = np.random.RandomState(0)
    for i in range(4):
        Image.fromarray(rng.randint(0, 255, (90, 120, 3), dtype=np.uint8)).save(root / f"{i}.png")
    port = 29950 + (os.getpid() % 40)
    mp.spawn(_coach_worker, args=(2, port, str(root), str(tmp_path / "out")), nprocs=2, join=True)
    out = tmp_path / "out" / "dp"
    assert (out / "mapper-final_object.pt").exists()
    assert (out / "validation-iter_2-denoisesteps_2_upsample_1_imgs_t2i_0.png").exists()


def test_world2_step_is_the_world1_graph_plus_one_collective_node():
    """north_star's exchange on the RCCL path: with a stream-ordered library communicator the data-parallel step is ONE
    hipGraph — the one-GPU launch list, one collective node, the same fused AdamW — not graph A / host all-reduce / graph B.
    A test box has one GPU, so the communicator is a real world-size-1 RCCL communicator (sum over ranks = identity)
    handed to an engine that otherwise believes world_size = 2 (grad_div 2)."""
    from view_neti_amd import ops, parallel
    comm = parallel.RcclComm(0, 1, exchange=lambda b: b)
    torch.manual_seed(0)
    cfg, e1 = _build(1, 1, False)
    torch.manual_seed(0)
    _, e2 = _build_x(comm)
    sig = lambda eng: [(getattr(f, "func", f).__name__, tuple(sorted((k, v) for k, v in getattr(f, "keywords", {}).items()
                                                                   if isinstance(v, (int, float, bool, type(None))))))
                       for f in eng.launches()]
    assert sig(e1) == sig(e2), "the N > 1 step must replay the N = 1 launch list"
    for eng in (e1, e2):
        _feed(cfg, eng, 0, 0, False)
        eng.capture()
    assert e1.graph_b is None and e2.graph_b is None and e2.exchange_in_graph, "world 2 on RCCL: one graph"
    assert float(e2.hyper[5]) == 2.0
    # replay: exactly one collective per step; identical arithmetic to the eager world-2 step (same launches, same order)
    c0 = parallel.COLLECTIVE_CALLS
    for step in range(2):
        _feed(cfg, e2, step, 0, False)
        assert e2.step() is True
    torch.cuda.synchronize()
    assert parallel.COLLECTIVE_CALLS - c0 == 2
    p_graph = e2.params.clone()
    torch.manual_seed(0)
    e3 = _build_x(comm)[1]
    for step in range(2):
        _feed(cfg, e3, step, 0, False)
        assert e3.step_eager() is True
    torch.cuda.synchronize()
    assert torch.equal(p_graph, e3.params), "captured exchange differs from the eager one"
    assert not torch.equal(p_graph, e1.params)
    comm.close()


def _build_x(comm):
    """_build(world 2) with an injected communicator"""
    from view_neti_amd.engine import step as step_mod
    orig = step_mod.TrainStepEngine.__init__

    def patched(self, *a, **kw):
        kw.setdefault("exchange", comm)
        return orig(self, *a, **kw)

    step_mod.TrainStepEngine.__init__ = patched
    try:
        return _build(2, 1, False)
    finally:
        step_mod.TrainStepEngine.__init__ = orig
