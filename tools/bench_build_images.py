"""CLI-level rate of `search.py build-images` against `compress.py` on the same files, in one process: N synthetic JPEG files of
size x size on local disk (the corpus of tools/cli_throughput.py) -> each command twice (the second pass runs with warm tile and
page caches) -> the commands' own JSON records.  Set-up differs (compress builds the 1.24 B-parameter codec as well), so the comparison is
`loop_images_per_s`: for build-images its record's own (loader header pass and plan, every batch, the last sync); for compress its
`cli_images_per_s`, whose clock starts after the models are built and covers the same span plus the container writes.  build-images indexes the folder with the CLIP tower alone; compress is the only
other way to an index, and also writes the containers.
usage: python tools/bench_build_images.py [N=640] [size=256] [batch=32] [--no_compress]"""
import io
import json
import os
import sys
import tempfile
import time
from contextlib import redirect_stdout

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from PIL import Image

import sgic_amd  # noqa
from sgic_amd import compress, search
from sgic_amd.data import synth_images

FLAGS = [a for a in sys.argv[1:] if a.startswith("--")]
POS = [a for a in sys.argv[1:] if not a.startswith("--")]
N = int(POS[0]) if len(POS) > 0 else 640
S = int(POS[1]) if len(POS) > 1 else 256
B = int(POS[2]) if len(POS) > 2 else 32
if not torch.cuda.is_available():
    sys.exit("bench_build_images needs the GPU")


def run(leg, main, argv, rep):
    buf = io.StringIO()
    t0 = time.perf_counter()
    with redirect_stdout(buf):
        rc = main(argv)
    rec = json.loads(buf.getvalue().strip().splitlines()[-1])
    rec.setdefault("loop_images_per_s", rec["cli_images_per_s"])     # compress: its rate's clock already starts after the model build
    rec.update(leg=leg, rc=rc, pass_=rep, size=S, wall_incl_model_build_s=round(time.perf_counter() - t0, 2))
    print(json.dumps(rec), flush=True)


with tempfile.TemporaryDirectory() as tmp:
    src = os.path.join(tmp, "in")
    os.makedirs(src)
    base = ((synth_images(64, S, S, 3) * 0.5 + 0.5) * 255).round().byte().permute(0, 2, 3, 1).numpy()
    for i in range(N):
        Image.fromarray(np.ascontiguousarray(np.roll(base[i % 64], i // 64, axis=0))).save(os.path.join(src, f"im{i:05d}.jpg"), quality=90)
    for rep in range(2):
        run("build-images", search.main, ["build-images", "--image_dir", src, "--index_dir", os.path.join(tmp, f"ix{rep}"),
                                          "--batch_size", str(B)], rep)
        if "--no_compress" not in FLAGS:
            run("compress", compress.main, ["--dataset_dir", src, "--save_dir", os.path.join(tmp, f"out{rep}"), "--batch_size", str(B)], rep)
