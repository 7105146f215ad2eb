#!/usr/bin/env python3
"""`python evaluate.py --originals <dir> --bitstreams <dir of .c2df> [--recon_dir <dir>] [--out report.jsonl]` -- bpp, PSNR, SSIM and
MS-SSIM of every image of a compressed folder, measured on the GPU."""
import sys
import sgic_amd  # noqa: F401
from sgic_amd.evaluate import main
sys.exit(main())
