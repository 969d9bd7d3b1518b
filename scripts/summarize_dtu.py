"""Summarize the DTU novel-view metrics (LPIPS, SSIM, PSNR per seed) of runs evaluated with scripts/inference.py,
averaged over the runs of each dtu_subset; the reference's scripts/summarize_dtu.py with its paths as arguments.

    python scripts/summarize_dtu.py --runs 'results/*_subs_1_*' 'results/*_subs_3_*' --iterations 1500 3000 \
        --lpips_vgg_weights vgg16-397923af.pth --lpips_lin_weights vgg.pth --out summarize_dtu.csv
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from view_neti_amd.compat.summarize_dtu import main  # noqa: E402

if __name__ == "__main__":
    main()
