"""GPU: decompress.py --format jpg --progressive with the SMALL model writes Pillow's progressive=True files of the PNG run's pixels;
without the flag the jpg and jpg --optimize outputs are what they were."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_enc_opt_ref as oref  # noqa: E402
import jpeg_enc_prog_ref as pref  # noqa: E402
import jpeg_enc_ref as eref  # noqa: E402
import quality_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [(256, 256)] * 3 + [(200, 300)]


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """compress and decompress (PNG) the four images of tests/test_gpu_evaluate_anchor.py once"""
    from PIL import Image
    import sgic_amd  # noqa: F401
    from sgic_amd import compress, decompress
    root = tmp_path_factory.mktemp("decompress_prog")
    src, out = root / "imgs", root / "out"
    src.mkdir()
    for i, (h, w) in enumerate(SIZES):
        Image.fromarray(ref.texture(np.random.default_rng(40 + i), h, w)).save(src / f"im{i}.png")
    assert compress.main(["--dataset_dir", str(src), "--save_dir", str(out), "--small", "--batch_size", "4"]) == 0
    assert decompress.main(["--dataset_dir", str(out / "bitstreams"), "--save_dir", str(out), "--small"]) == 0
    return {"root": root, "out": out}


def _pixels(run, i):
    from PIL import Image
    return np.array(Image.open(run["out"] / "results" / f"im{i}.png").convert("RGB"))


def _decompress(run, name, *flags):
    import sgic_amd  # noqa: F401
    from sgic_amd import decompress
    dst = run["root"] / name
    assert decompress.main(["--dataset_dir", str(run["out"] / "bitstreams"), "--save_dir", str(dst), "--small", "--format", "jpg", *flags]) == 0
    assert sorted(os.listdir(dst / "results")) == [f"im{i}.jpg" for i in range(4)]
    return [(dst / "results" / f"im{i}.jpg").read_bytes() for i in range(4)]


def test_progressive_files_are_pillows(run):
    got = _decompress(run, "prog", "--quality", "80", "--progressive")
    for i in range(4):
        assert got[i] == pref.pillow_bytes(_pixels(run, i), 80, 2), i
    assert _decompress(run, "prog_opt", "--quality", "80", "--progressive", "--optimize") == got      # as in Pillow


def test_progressive_with_subsampling_and_max_side(run):
    from PIL import Image
    got = _decompress(run, "prog_small", "--quality", "60", "--subsampling", "0", "--max_side", "100", "--progressive")
    for i, (h, w) in enumerate(SIZES):
        small = Image.fromarray(_pixels(run, i)).resize((100, 100) if h == w else (100, 67), Image.LANCZOS)
        assert got[i] == pref.pillow_bytes(np.array(small), 60, 0), i


def test_without_the_flag_nothing_changes(run):
    plain = _decompress(run, "plain", "--quality", "80")
    opt = _decompress(run, "opt", "--quality", "80", "--optimize")
    for i in range(4):
        assert plain[i] == eref.pillow_bytes(_pixels(run, i), 80, 2), i
        assert opt[i] == oref.pillow_bytes(_pixels(run, i), 80, 2), i


def test_progressive_needs_jpg(run, capsys, monkeypatch):
    import sgic_amd  # noqa: F401
    from sgic_amd import codec, decompress

    def no_model(*a, **k):
        raise AssertionError("a model was built")
    monkeypatch.setattr(codec, "Codec", no_model)
    for fmt in (["--format", "png"], []):
        with pytest.raises(SystemExit) as e:
            decompress.main(["--dataset_dir", str(run["out"] / "bitstreams"), "--save_dir", str(run["root"] / "no"), "--small", "--progressive"] + fmt)
        assert e.value.code not in (0, None) and "--format jpg" in capsys.readouterr().err
    assert not (run["root"] / "no").exists()
