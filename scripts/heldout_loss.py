"""Held-out diffusion loss of the saved checkpoints of a run (compat/heldout.py): the evaluation `eval.heldout_loss_steps`
runs during training, on `mapper-steps-N_{object,view}.pt` after the fact — same plan, same fixed noise, one forward-only
engine for all iterations.

    python scripts/heldout_loss.py --input_dir <run> --iterations [1500,3000] \
        [--heldout_loss_timesteps 4] [--heldout_loss_seed 0] [--eval_placeholder_object_tokens ["<scan65>"]] \
        [--use_ema true]   (the averaged mappers mapper-ema-steps-N_* of a run with optim.ema_decay)
        [--heldout_loss_masked true]   ("loss_masked" beside every loss: the run's data.mask_dir object masks)

Appends one line per iteration to <run>/heldout-loss-offline.jsonl and prints iteration x train / test.
"""
import os
import sys
from dataclasses import dataclass, field
from pathlib import Path
from typing import List, Optional

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from view_neti_amd.compat import config as cfgmod  # noqa: E402


@dataclass
class HeldoutLossConfig:
    input_dir: Optional[Path] = None
    iterations: List[int] = field(default_factory=list)
    eval_placeholder_object_tokens: List[str] = field(default_factory=list)  # mode 3, as scripts/inference.py
    heldout_loss_timesteps: int = 4
    heldout_loss_seed: int = 0
    use_ema: bool = False
    heldout_loss_masked: bool = False


def main(args=None):
    cfg = cfgmod.parse(HeldoutLossConfig, args)
    if cfg.input_dir is None or not cfg.iterations:
        raise SystemExit("heldout_loss: --input_dir and --iterations are required")
    from view_neti_amd.compat import heldout
    records = heldout.offline(cfg.input_dir, cfg.iterations, cfg.eval_placeholder_object_tokens,
                              cfg.heldout_loss_timesteps, cfg.heldout_loss_seed, use_ema=cfg.use_ema,
                              masked=cfg.heldout_loss_masked)
    print(heldout.format_table(records))
    return records


if __name__ == "__main__":
    main()
