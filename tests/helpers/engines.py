"""The tiny `TrainStepEngine` the engine-level GPU tests train, built in one place: the mapper arguments (a pure CPU
function, so the numbers can be compared without a GPU), the engine around them, the three ways the tests feed it, and the
state snapshots they compare.

pytest does not rewrite the asserts of a helper module: every assert here carries its message."""
import contextlib

import torch

from view_neti_amd.engine.step import TrainStepEngine  # (imports ctypes bindings only: no library is loaded, no GPU touched)

# ------------------------------------------------------------------------------------------------ the state field tuples
FIELDS = TrainStepEngine._STATE                                  # what state_dict() holds
STATE = tuple(f for f in FIELDS if f != "hyper")                 # ... without the hyper-parameters (the lr is scheduled)
STATE_PLUS = FIELDS + ("grads", "loss_sum")                      # ... with what an evaluation must leave alone too

# ------------------------------------------------------------------------------------------------ mapper arguments (CPU)
# The object states, then the view state, are perturbed with ONE seeded generator in that order.  Their initialisation
# and the two Fourier matrices draw from (and reseed) the GLOBAL generator, and the call sites differ in the order of
# those draws; each order gives other numbers, and the oracle-parity and bit-equality tests pin them:
W_ENC_FIRST = "w_enc-first"        # w_enc; each object state initialised and perturbed; w_enc_view; the view state
INIT_ALL_FIRST = "init-all-first"  # w_enc; every state initialised; then every state perturbed; w_enc_view last
STATES_FIRST = "states-first"      # each state initialised and perturbed (objects, view); w_enc_view; w_enc last


def mapper_args(cfg_name, n_obj=1, with_view=False, perturb_seed=1, fork_rng=False, order=W_ENC_FIRST):
    """-> (object mapper state, or the list of them if n_obj > 1; w_enc; the view mapper's keyword arguments, {} without)

    fork_rng: the global `torch.manual_seed(0)` and the draws under it leave the global generator as they found it (the
    w_enc_view of INIT_ALL_FIRST is drawn after that, and reseeds it, as it always did)."""
    from view_neti_amd import sd_config as sc
    from view_neti_amd.mapper import fourier_frequencies, init_mapper_state
    D = sc.CONFIGS[cfg_name]().clip.hidden_size
    gen = torch.Generator().manual_seed(perturb_seed)
    init = lambda: init_mapper_state(64, 64, D)
    perturb = lambda sd: {k: v + 0.05 * torch.randn(v.shape, generator=gen) for k, v in sd.items()}
    enc_obj = lambda: fourier_frequencies([0.03, 2.0], 64, 0)
    enc_view = lambda: fourier_frequencies([0.03, 2.0] + [0.5] * 12, 64, 0)
    n, w_enc_v = n_obj + bool(with_view), None
    with torch.random.fork_rng(devices=[]) if fork_rng else contextlib.nullcontext():
        torch.manual_seed(0)
        if order == W_ENC_FIRST:
            w_enc = enc_obj()
            states = [perturb(init()) for _ in range(n_obj)]
            if with_view:
                w_enc_v = enc_view()
                states.append(perturb(init()))
        elif order == INIT_ALL_FIRST:
            w_enc = enc_obj()
            states = [init() for _ in range(n)]
        elif order == STATES_FIRST:
            states = [perturb(init()) for _ in range(n)]
            if with_view:
                w_enc_v = enc_view()
            w_enc = enc_obj()
        else:
            raise ValueError(f"unknown draw order {order!r}")
    if order == INIT_ALL_FIRST:
        states = [perturb(sd) for sd in states]
        if with_view:
            w_enc_v = enc_view()
    view = dict(mapper_view=states[n_obj], w_enc_view=w_enc_v, norm_scale_view=0.35, alpha_view=0.3) if with_view else {}
    return (states[0] if n_obj == 1 else states[:n_obj]), w_enc, view


def build_train_engine(cfg_name, B, H, W, n_obj=1, with_view=False, perturb_seed=1, fork_rng=False, order=W_ENC_FIRST,
                       loud_seed=None, **kw):
    """-> cfg, eng, (uw, vw, cw), object state(s), w_enc, view keyword arguments.  The synthetic weights of the tiny families
    stay on the host (the engine packs them), the full-size ones are made on the device; **kw goes to the engine.
    loud_seed: the 1-D tensors of the three frozen models are replaced by helpers/loud_weights.py's (seeds loud_seed,
    loud_seed + 1, loud_seed + 2 for UNet, VAE, CLIP); the returned dicts are the ones the engine was built on."""
    from view_neti_amd import sd_config as sc, synth
    cfg = sc.CONFIGS[cfg_name]()
    dev = "cpu" if cfg_name.startswith("tiny") else "cuda"
    uw, vw, cw = synth.unet_weights(cfg.unet, device=dev), synth.vae_weights(cfg.vae, device=dev), synth.clip_weights(cfg.clip, device=dev)
    if loud_seed is not None:
        from helpers.loud_weights import loud
        uw, vw, cw = loud(uw, loud_seed), loud(vw, loud_seed + 1), loud(cw, loud_seed + 2)
    sd, w_enc, extra = mapper_args(cfg_name, n_obj, with_view, perturb_seed, fork_rng, order)
    eng = TrainStepEngine(cfg, uw, vw, cw, B, H, W, sd, w_enc, 0.4, 0.2, **extra, **kw)
    return cfg, eng, (uw, vw, cw), sd, w_enc, extra


def build_device_rng_engine(mode3=False, accum=1, B=2, H=64, W=64, lr=3e-3, **kw):
    """-> cfg, eng: the tiny engine with everything that makes its state non-trivial switched on — device RNG (seed 5),
    nested dropout, and a GradScaler that grows every 3 clean steps; one object mapper, or (mode3) three and the view mapper"""
    kw.setdefault("growth_interval", 3)
    cfg, eng, _, _, _, _ = build_train_engine("tiny", B, H, W, n_obj=3 if mode3 else 1, with_view=mode3, perturb_seed=7,
                                              order=STATES_FIRST, lr=lr, grad_accum=accum, device_rng=True,
                                              nested_dropout_prob=0.5, seed=5, **kw)
    return cfg, eng


# ------------------------------------------------------------------------------------------------ feeders
SCENES = (0, 2, 0, 2)


def feed_device_rng(cfg, eng, step, micro, mode3, scenes=SCENES, stride=2, n_images=4):
    """for an engine that draws its own noise.  Micro-batch `micro` of optimizer step `step` (number stride * step + micro):
    two of `n_images` fixed images (the pixels behind a dataset index never change: what the moment cache relies on),
    captions and camera parameters that differ per micro-batch, the scene of the step"""
    from view_neti_amd import synth
    B, H, W = eng.B, eng.H, eng.W
    k = stride * step + micro
    idx = [(2 * k) % n_images, (2 * k + 1) % n_images]
    px = torch.cat([synth.gaussian((1, 3, H, W), 50 + i).clamp(-1, 1) for i in idx])
    ph, phv = cfg.clip.vocab_size - 3, cfg.clip.vocab_size - 4
    ids = synth.input_ids(B, ph, cfg.clip.vocab_size, view_placeholder_id=phv if mode3 else None)
    kw = dict(image_idx=idx) if eng.n_cache else {}
    if mode3:
        eng.set_batch(px, ids, torch.full((B,), ph), torch.full((B,), phv), synth.gaussian((B, 12), 100 + k).clamp(-1, 1),
                      object_index=scenes[step], **kw)
    else:
        eng.set_batch(px, ids, torch.full((B,), ph), **kw)


def feed_host_noise(cfg, eng, step, shard, mode3, scenes):
    """for an engine with device_rng=False.  Micro-batch `shard` (= the rank in a data-parallel run) of optimizer step
    `step`: host-supplied data and noise"""
    from view_neti_amd import synth
    B, H, W = eng.B, eng.H, eng.W
    s = 100 * step + 10 * shard
    ph, phv = cfg.clip.vocab_size - 3, cfg.clip.vocab_size - 4
    ids = synth.input_ids(B, ph, cfg.clip.vocab_size, view_placeholder_id=phv if mode3 else None)
    px = synth.gaussian((B, 3, H, W), s + 1).clamp(-1, 1)
    if mode3:
        eng.set_batch(px, ids, torch.full((B,), ph), torch.full((B,), phv), synth.gaussian((B, 12), s + 2).clamp(-1, 1),
                      object_index=scenes[step])
    else:
        eng.set_batch(px, ids, torch.full((B,), ph))
    t = torch.randint(0, 1000, (B,), generator=torch.Generator().manual_seed(s + 3))
    eng.set_noise(synth.gaussian((B, 4, H // 8, W // 8), s + 4), synth.gaussian((B, 4, H // 8, W // 8), s + 5), t)


def batch_dict(cfg, B, H=64, W=64, seed=0):
    """one object + view batch with its noise as a dict, for tests that feed the same batch for training and evaluation"""
    from view_neti_amd import synth
    V = cfg.clip.vocab_size
    ph, phv = V - 3, V - 4
    return dict(px=synth.pixel_values(B, H, W, seed=1 + seed), ids=synth.input_ids(B, ph, V, view_placeholder_id=phv),
                po=torch.full((B,), ph), pv=torch.full((B,), phv), vp=synth.gaussian((B, 12), 9 + seed).clamp(-1, 1),
                t=synth.timesteps(B, seed=2 + seed), eps=synth.gaussian((B, 4, H // 8, W // 8), 3 + seed),
                noise=synth.gaussian((B, 4, H // 8, W // 8), 4 + seed))


def feed_dict(eng, b, for_eval=False, **kw):
    eng.set_batch(b["px"], b["ids"], b["po"], b["pv"], b["vp"], for_eval=for_eval, **kw)


def run_steps(cfg, eng, steps, mode3, feed):
    """the optimizer steps `steps`, each eng.grad_accum micro-steps fed by feed(cfg, eng, step, micro, mode3)"""
    for s in steps:
        for m in range(eng.grad_accum):
            feed(cfg, eng, s, m, mode3)
            closed = eng.step()
            assert closed is (m == eng.grad_accum - 1), f"step {s} micro {m}: eng.step() returned {closed!r}"


def snapshot(eng, fields):
    torch.cuda.synchronize()
    return {f: getattr(eng, f).detach().cpu().clone() for f in fields}


# ------------------------------------------------------------------------------------------------ six captured steps
FORMS = {"one-mapper": (False, 1), "mode3": (True, 1), "accum2": (False, 2)}  # form -> (mode3, grad_accum)


def feed_six(cfg, eng, step, micro, mode3):
    feed_device_rng(cfg, eng, step % len(SCENES), micro, mode3)  # (the scene list has 4 entries: steps 4, 5 repeat 0, 1)


_RUNS = {}


def six_steps(form, **kw):
    """the state after 6 captured optimizer steps of build_device_rng_engine(*FORMS[form], **kw), its telemetry rows and its
    scaler; computed once per (form, arguments) and left unchanged, for every test file that compares against it"""
    key = (form, tuple(sorted(kw.items())))
    if key not in _RUNS:
        mode3, accum = FORMS[form]
        cfg, eng = build_device_rng_engine(mode3, accum, **kw)
        feed_six(cfg, eng, 0, 0, mode3)
        eng.capture()
        run_steps(cfg, eng, range(6), mode3, feed_six)
        rows = eng.read_telemetry() if eng.telemetry_rows else None
        _RUNS[key] = (snapshot(eng, STATE), rows, eng.scaler.cpu().clone())
    return _RUNS[key]
