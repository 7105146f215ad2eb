#!/usr/bin/env python3
"""Rate and distortion of a compressed folder: bpp, PSNR, SSIM and MS-SSIM of every image against its original, measured on the GPU
(quality.measure; the measures of the reference's taming/modules/losses/quality.py that need no network weights).

  evaluate.py --originals imgs --bitstreams out/bitstreams      decodes the containers (as decompress.py does, but the u8 image stays
                                                                on the device and no PNG is written)
  evaluate.py --originals imgs --recon_dir out/results          compares two folders; no model is built (--bitstreams adds the rate)

  evaluate.py ... --bitstreams out/bitstreams --anchor jpeg      adds a JPEG anchor at matched rate to every record: the original is
                                                                encoded on the GPU at qualities 1..95 (jpeg_enc), the largest
                                                                quality whose file is not larger than the container is kept, decoded
                                                                on the GPU (jpeg.JpegBatch) and measured like the reconstruction
  evaluate.py ... --anchor_quality Q                            the anchor at a fixed quality (needs no --bitstreams)
  evaluate.py ... --anchor_optimize                             the anchor with Huffman tables fitted to every image (Pillow's
                                                                optimize=True): the ladder, the pick and the kept file
  evaluate.py ... --anchor_scales R [R ...]                     the anchor at reduced resolution, what a JPEG user does at low rates:
                                                                for every R the original is reduced to ceil(H / R) x ceil(W / R)
                                                                (Lanczos, ops.resize_u8), coded as above, decoded and enlarged back
                                                                (bicubic); every image keeps the R with the highest PSNR among those
                                                                with a quality that fits its container.  The anchor then carries
                                                                "scale", "coded_height", "coded_width", the summary
                                                                "anchor_scale_counts".  With --anchor_quality: exactly one R
  evaluate.py ... --lpips_ckpt P [P ...]                        adds "lpips" to every record, to its anchor and to the summary: LPIPS
                                                                with the VGG16 trunk (lpips.LpipsVGG) on the same u8 tensors; P: one
                                                                or more state dict files that together hold the trunk and the lin
                                                                layers (lpips.load_weights)
  evaluate.py ... --lpips_alex_ckpt P [P ...]                   adds "lpips_alex" in the same places (directly after "lpips" where
                                                                both are asked for): LPIPS with the AlexNet trunk, the `lpips` of the
                                                                reference's Quality_Model (lpips_alex.LpipsAlex); P: state dict
                                                                file(s) with the trunk and the lin layers (lpips_alex.load_weights)
  evaluate.py ... --dists_ckpt P [P ...]                        adds "dists" in the same places (after "lpips" where both are asked
                                                                for): DISTS with the VGG16 trunk (dists.DistsVGG); P: state dict
                                                                file(s) with the trunk, alpha and beta (dists.load_weights)
  evaluate.py ... --fid_ckpt P [P ...] [--fid_patch 256]        adds "fid", "kid", "kid_std", "fid_patches" and "fid_skipped" to the
                                                                summary (and "anchor_fid", "anchor_kid", "anchor_kid_std" with an
                                                                anchor): FID and KID between the set of originals and the set of
                                                                reconstructions on pytorch-fid's Inception-v3 (fid.InceptionFID), over
                                                                the 256 x 256 windows of the HiFiC protocol (fid.patch_grid;
                                                                --fid_patch 0: whole images); P: state dict file(s) of the Inception
                                                                (torchvision's or pytorch-fid's keys, fid.load_weights).  The
                                                                per-image lines do not change
  evaluate.py ... --clip_ckpt P                                 retrieval fidelity: adds "clip_sim" to every record (and to its
                                                                anchor), the cosine between the CLIP image tower's vectors of the
                                                                original and of the reconstruction, and "clip_sim", "clip_recall@1",
                                                                "clip_recall@5", "clip_recall@10", "clip_mrr", "clip_median_rank" to
                                                                the summary ("anchor_clip_*" with an anchor): every reconstruction
                                                                searches the u8 codes of all evaluated originals for its own original
                                                                (search.CodeIndex.rank_vectors).  With --bitstreams also
                                                                "clip_code_match" per record and "clip_code_mismatch" in the summary:
                                                                whether the code in the container is the code P gives the original.
                                                                P: the state dict compress.py --clip_ckpt takes (--small: the TINY
                                                                tower)
  evaluate.py ... --niqe_params P                               adds "niqe" (of the reconstruction) and "niqe_orig" (of the original)
                                                                to every record, "niqe" to its anchor and their means to the summary
                                                                ("anchor_niqe" with an anchor): the no-reference NIQE score on the
                                                                same u8 tensors (niqe.Niqe), null for an image with fewer than two
                                                                usable 96 x 96 blocks; P: the pristine model, an .npz with
                                                                mu_pris_param and cov_pris_param (BasicSR's file, or the output of
                                                                `python -m sgic_amd.niqe fit`) or MATLAB's .mat
  evaluate.py ... --hvs                                         adds "vifp", "gmsd", "psnr_hvs" and "psnr_hvs_m" to every record and
                                                                to its anchor, directly after "ms_ssim_db", and their means to the
                                                                summary ("anchor_*" with an anchor): pixel-domain VIF, gradient
                                                                magnitude similarity deviation and PSNR-HVS / PSNR-HVS-M on fp64 luma
                                                                (quality.measure_hvs); they need no file.  An image too small for a
                                                                measure (VIFp: a side below 41; PSNR-HVS: below 8) carries null there
                                                                and is counted in the summary's "hvs_skipped"
  evaluate.py ... --fsim                                        adds "fsim" and "fsimc" to every record and to its anchor, directly
                                                                after "ms_ssim_db" (after "psnr_hvs_m" with --hvs), and their means
                                                                to the summary ("anchor_*" with an anchor): the feature similarity
                                                                index on phase congruency and gradient magnitude, and its colour
                                                                variant with the I / Q chroma term (quality.fsim); they need no
                                                                file.  An image FSIM refuses (a side below 2, a reduced longer side
                                                                above 2048) carries null and is counted in "fsim_skipped"

One JSON line per image, sorted by name, to --out (default: stdout); a summary line to stderr, which is also the last line of --out.
Originals and reconstructions are matched by file stem."""
import argparse
import json
import math
import os
import sys
from glob import glob

import numpy as np
import torch

from .quality import FSIM_FIELDS, HVS_FIELDS      # --hvs, then --fsim: directly after FIELDS, in a record and in its anchor

torch.set_grad_enabled(False)

FIELDS = ("psnr", "ssim", "ms_ssim", "ms_ssim_db")
PAIR_METRICS = ("lpips", "lpips_alex", "dists")      # the perceptual pair metrics, in the order of their keys in a record


def to_u8_hwc_device(x_chw_01):
    """decompress.to_u8_hwc (torchvision's save_image arithmetic) without the copy to the host: the bytes of the PNG"""
    return x_chw_01.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(torch.uint8).contiguous()


def load_rgb(path):
    """-> (H, W, 3) u8, or the exception that reading raised (the caller reports it: this runs on a pool thread)"""
    from PIL import Image
    try:
        return np.array(Image.open(path).convert("RGB"), dtype=np.uint8)
    except Exception as e:   # noqa: BLE001 -- any unreadable file is a [SKIP] line, not the end of the run
        return e


def by_stem(paths):
    from .compress import stem_of
    return {stem_of(p): p for p in sorted(paths)}


def _json_number(v):
    if v is None:
        return None
    v = float(v)
    return ("inf" if v > 0 else "-inf") if math.isinf(v) else v


def summarise(records, fid_sets=None, clip_sets=None):
    """the summary line: count and the fp64 means of bpp, psnr (finite values), ms_ssim; ms_ssim_db of the mean ms_ssim; the mean of
    vifp, gmsd, psnr_hvs, psnr_hvs_m (finite values) and the count hvs_skipped of records with a null among them when the records
    carry them (--hvs); the mean of fsim, fsimc and the count fsim_skipped likewise (--fsim); the mean of lpips, lpips_alex and dists when the records carry them; clip_sets (ClipSets, --clip_ckpt): its
    keys after the perceptual means (the anchor's after the anchor's); fid_sets (FidSets, --fid_ckpt): its keys after all the others"""
    def mean(vals):
        return float(np.mean(np.array(vals, dtype=np.float64))) if vals else None
    ms = mean([r["ms_ssim"] for r in records if r["ms_ssim"] is not None])
    with np.errstate(divide="ignore"):
        db = None if ms is None else float(0.0 - 10.0 * np.log10(1.0 - ms))
    out = {"images": len(records), "bpp": mean([r["bpp"] for r in records if r["bpp"] is not None]),
           "psnr": mean([r["psnr"] for r in records if isinstance(r["psnr"], float)]), "ms_ssim": ms, "ms_ssim_db": _json_number(db)}
    if any("vifp" in r for r in records):
        for k in HVS_FIELDS:
            out[k] = mean([r[k] for r in records if isinstance(r.get(k), float)])
        out["hvs_skipped"] = sum(1 for r in records if any(r.get(k) is None for k in HVS_FIELDS))
    if any("fsim" in r for r in records):
        for k in FSIM_FIELDS:
            out[k] = mean([r[k] for r in records if isinstance(r.get(k), float)])
        out["fsim_skipped"] = sum(1 for r in records if any(r.get(k) is None for k in FSIM_FIELDS))
    for k in PAIR_METRICS:
        if any(k in r for r in records):
            out[k] = mean([r[k] for r in records if r.get(k) is not None])
    if clip_sets is not None:
        out["clip_sim"] = mean([r["clip_sim"] for r in records])
        out.update(clip_sets.summary("recon", records, "clip_"))
        if any("clip_code_match" in r for r in records):
            out["clip_code_mismatch"] = sum(1 for r in records if r.get("clip_code_match") is False)
    anchors = [r["anchor"] for r in records if "anchor" in r]
    if anchors:      # the same means over the anchors; over_rate counts the images whose smallest JPEG is larger than the container
        ams = mean([a["ms_ssim"] for a in anchors if a["ms_ssim"] is not None])
        with np.errstate(divide="ignore"):
            adb = None if ams is None else float(0.0 - 10.0 * np.log10(1.0 - ams))
        out.update({"anchor_bpp": mean([a["bpp"] for a in anchors]),
                    "anchor_psnr": mean([a["psnr"] for a in anchors if isinstance(a["psnr"], float)]), "anchor_ms_ssim": ams,
                    "anchor_ms_ssim_db": _json_number(adb), "anchor_over_rate": sum(1 for a in anchors if a["over_rate"])})
        if any("vifp" in a for a in anchors):
            for k in HVS_FIELDS:
                out["anchor_" + k] = mean([a[k] for a in anchors if isinstance(a.get(k), float)])
        if any("fsim" in a for a in anchors):
            for k in FSIM_FIELDS:
                out["anchor_" + k] = mean([a[k] for a in anchors if isinstance(a.get(k), float)])
        for k in PAIR_METRICS:
            if any(k in a for a in anchors):
                out["anchor_" + k] = mean([a[k] for a in anchors if a.get(k) is not None])
        if clip_sets is not None:
            out["anchor_clip_sim"] = mean([a["clip_sim"] for a in anchors])
            out.update(clip_sets.summary("anchor", [r for r in records if "anchor" in r], "anchor_clip_"))
        if any("scale" in a for a in anchors):      # --anchor_scales: how many images kept which scale, the last anchor key
            out["anchor_scale_counts"] = {str(r): sum(1 for a in anchors if a.get("scale") == r)
                                          for r in sorted({a["scale"] for a in anchors if "scale" in a})}
    if fid_sets is not None:
        out.update(fid_sets.summary())
    if any("niqe" in r for r in records):      # --niqe_params: after every other key
        out["niqe"] = mean([r["niqe"] for r in records if r.get("niqe") is not None])
        out["niqe_orig"] = mean([r["niqe_orig"] for r in records if r.get("niqe_orig") is not None])
        if anchors:
            out["anchor_niqe"] = mean([a["niqe"] for a in anchors if a.get("niqe") is not None])
    return out


class FidSets:
    """--fid_ckpt: the Inception features of the originals, the reconstructions and (with an anchor) the decoded anchors over the same
    windows (fid.patch_grid of every image), accumulated on the device; FID and KID once at the end"""

    def __init__(self, ckpt, patch, device):
        from . import fid
        self.fid, self.patch = fid, int(patch)
        self.model = fid.InceptionFID(ckpt, device)
        self.orig, self.recon, self.anchor = fid.FeatureStats(), fid.FeatureStats(), fid.FeatureStats()
        self.skipped = 0

    def windows(self, a):
        """a (B, H, W, 3) -> the descriptors of the batch, None when the images give no window (counted as skipped)"""
        B, H, W, _ = a.shape
        desc = self.fid.descriptors(B, H, W, self.patch)
        if not len(desc):
            self.skipped += B
            return None
        return desc

    def add(self, which, images, desc):
        getattr(self, which).add(self.model.features(images, desc))

    def _pair(self, x, y):
        if x.n < 2 or y.n < 2:
            return None, None, None
        X, Y = x.features(), y.features()
        k, k_std = self.fid.kid(X, Y)
        return self.fid.fid(X, Y), k, k_std

    def summary(self):
        n = self.orig.n
        if 0 < n < self.fid.DIM:
            print(f"[WARN] FID over {n} windows: with fewer than {self.fid.DIM} samples the covariances are rank-deficient and the number "
                  "is biased; compare it only with numbers over the same count", file=sys.stderr)
        f, k, k_std = self._pair(self.orig, self.recon)
        out = {"fid": f, "kid": k, "kid_std": k_std, "fid_patches": n, "fid_skipped": self.skipped}
        if self.anchor.n:
            f, k, k_std = self._pair(self.orig, self.anchor)
            out.update({"anchor_fid": f, "anchor_kid": k, "anchor_kid_std": k_std})
        return out


class ClipSets:
    """--clip_ckpt: the CLIP image tower over the u8 tensors the other measures see.  Every original gives a unit vector and the u8
    code of it (ClipCodec.u8_to_codes: the decoded bytes as they are, the route of `search.py build-images`), every reconstruction and
    decoded anchor a unit vector; they are kept per image name, and at the end the reconstructions (anchors) search the codes of all
    originals for their own (search.CodeIndex.rank_vectors, the rank kernel).  stored_route_codes: the code compress.py writes into
    a container, which goes through the fp32 image (ClipCodec.batch_to_codes on u / 255 * 2 - 1) -- what a container's
    code is compared with"""

    def __init__(self, ckpt, small, device):
        from . import weights as W
        from .codec import ClipCodec
        from .compress import load_state
        from .config import CLIP_B32, CLIP_TINY
        ccfg = CLIP_TINY if small else CLIP_B32
        csd = load_state(ckpt, W.clip_spec, ccfg, 4321)
        if ckpt and not any(k.startswith("clip.") for k in csd):
            csd = {f"clip.{k}": v for k, v in csd.items()}
        self.clipc = ClipCodec(csd, ccfg, device)
        self.codes, self.units = {}, {"recon": {}, "anchor": {}}

    def embed(self, images):
        """(B, H, W, 3) u8 on the device -> (unit (B, D) fp32, codes (B, D) u8), both on the host"""
        B, H, W, _ = images.shape
        unit, codes = self.clipc.u8_to_codes(images.contiguous(), np.array([(H, W)] * B, dtype=np.int64))
        return unit.cpu().numpy(), codes.cpu().numpy()

    def stored_route_codes(self, images):
        from . import ops
        B, H, W, _ = images.shape
        return self.clipc.batch_to_codes(ops.u8hwc_to_f32chw_pad(images.contiguous()), H, W)[1].cpu().numpy()

    @staticmethod
    def cosine(u, v):
        """fp64 cosine per row of two (B, D) fp32 arrays"""
        u, v = u.astype(np.float64), v.astype(np.float64)
        return (u * v).sum(axis=1) / (np.sqrt((u * u).sum(axis=1)) * np.sqrt((v * v).sum(axis=1)))

    def summary(self, which, records, prefix):
        """the queries of set `which` for `records` against the codes of ALL evaluated originals, rows in name order"""
        from .search import CodeIndex, retrieval_summary
        names = sorted(self.codes)
        row = {n: j for j, n in enumerate(names)}
        asked = [r["name"] for r in records]
        if not asked:
            return {}
        ci = CodeIndex(np.stack([self.codes[n] for n in names]), names)
        rank, score = ci.rank_vectors(np.stack([self.units[which][n] for n in asked]), np.array([row[n] for n in asked], dtype=np.int64))
        s = retrieval_summary(rank, score, (1, 5, 10))
        return {prefix + k: s[k] for k in ("recall@1", "recall@5", "recall@10", "mrr", "median_rank")}


def _anchor_files(src_u8, budgets, subsampling, fixed_quality, optimize):
    """the anchor's pick and files for a batch as it is coded: src_u8 (B, h, w, 3) -> ([(quality, over_rate or None)], [bytes])"""
    from . import jpeg_enc
    B = src_u8.shape[0]
    if fixed_quality is None:
        sizes = jpeg_enc.ladder_sizes(src_u8, subsampling, optimize=optimize)
        picks = [jpeg_enc.pick_quality(dict(zip(jpeg_enc.LADDER, (int(v) for v in sizes[j]))), budgets[j]) for j in range(B)]
    else:
        picks = [(int(fixed_quality), None)] * B
    return picks, jpeg_enc.encode_batch(src_u8, [q for q, _ in picks], subsampling, optimize=optimize)


def choose_scale(candidates):
    """the rule of --anchor_scales for one image: candidates [(scale, over_rate, bytes, psnr)] in ascending scale -> the index of the
    one kept.  Among the scales where a quality fits the budget the highest PSNR (an infinite one wins), the smaller scale on a tie;
    if none fits, the smallest file, the smaller scale on a tie"""
    fits = [i for i, c in enumerate(candidates) if not c[1]]
    if fits:
        return max(fits, key=lambda i: (candidates[i][3], -i))
    return min(range(len(candidates)), key=lambda i: (candidates[i][2], i))


def jpeg_anchors(a_u8, budgets, subsampling, fixed_quality=None, pair_metrics=(), decoded_out=None, optimize=False, scales=None,
                 hvs=False, fsim=False):
    """the JPEG anchors of a batch of originals: a_u8 (B, H, W, 3) u8 on the device, budgets: the container size of every image in
    bytes (None: unknown) -> list of B anchor records.  Without fixed_quality every image is encoded at the qualities of
    jpeg_enc.LADDER and jpeg_enc.pick_quality takes the largest quality whose whole file fits the budget; the chosen files are decoded
    on the GPU and measured against the original.  Encode, decode and measurement stay on the device; sizes and numbers come back.
    pair_metrics: [(key, model)] in record order (lpips.LpipsVGG, lpips_alex.LpipsAlex, dists.DistsVGG): every record also carries
    `key`, the model's measure of the decoded anchor against the original.  decoded_out: a list that receives the decoded anchors
    (B, H, W, 3) u8 on the device (the FID of the anchor set).  optimize: sizes and files with Huffman tables fitted to every image
    (jpeg_enc's optimize); the records then carry "optimize": true after "subsampling".
    scales: the anchor at reduced resolution.  For every r of the list (ascending) the batch is reduced to resize.reduced_size(H, W, r)
    with Lanczos (ops.resize_u8; r = 1: the image as it is), picked and encoded as above against the same budgets, decoded, enlarged
    to (H, W) with bicubic and measured; every image keeps the scale choose_scale names.  The records then carry "scale",
    "coded_height" and "coded_width" after "subsampling" ("optimize"); "bytes" is the reduced file and "bpp" counts the original's
    pixels.
    hvs: every record also carries HVS_FIELDS (quality.measure_hvs of the decoded anchor), directly after FIELDS.
    fsim: and FSIM_FIELDS (quality.measure_fsim) after those."""
    from . import jpeg, ops, quality
    from .resize import reduced_size
    B, H, W, _ = a_u8.shape
    if scales is None:
        picks, files = _anchor_files(a_u8, budgets, subsampling, fixed_quality, optimize)
        decoded = jpeg.JpegBatch(files).decode(a_u8.device)
        coded = None
    else:
        per = []      # one entry per scale, ascending: what every image of the batch would get at it
        for r in sorted(int(r) for r in scales):
            h, w = reduced_size(H, W, r)
            src = a_u8 if r == 1 else ops.resize_u8(a_u8, h, w, "lanczos")
            pk, fl = _anchor_files(src, budgets, subsampling, fixed_quality, optimize)
            dec = jpeg.JpegBatch(fl).decode(a_u8.device)
            if r != 1:
                dec = ops.resize_u8(dec.contiguous(), H, W, "bicubic")
            per.append({"scale": r, "coded": (h, w), "picks": pk, "files": fl, "decoded": dec, "psnr": quality.measure(a_u8, dec)["psnr"]})
        kept = [per[choose_scale([(s["scale"], bool(s["picks"][j][1]), len(s["files"][j]), float(s["psnr"][j])) for s in per])]
                for j in range(B)]      # a fixed quality has no over_rate yet (None): its one scale is kept
        picks, files = [s["picks"][j] for j, s in enumerate(kept)], [s["files"][j] for j, s in enumerate(kept)]
        decoded = torch.stack([s["decoded"][j] for j, s in enumerate(kept)])
        coded = [(s["scale"], s["coded"]) for s in kept]
    if decoded_out is not None:
        decoded_out.append(decoded)
    m = quality.measure(a_u8, decoded)
    if hvs:
        m.update(quality.measure_hvs(a_u8, decoded))
    if fsim:
        m.update(quality.measure_fsim(a_u8, decoded))
    pm = [(k, model.measure(a_u8, decoded)) for k, model in pair_metrics]
    out = []
    for j, ((q, over), data) in enumerate(zip(picks, files)):
        if over is None:      # a fixed quality: over the rate if the container is known and smaller
            over = budgets[j] is not None and len(data) > budgets[j]
        rec = {"codec": "jpeg", "quality": q, "subsampling": int(subsampling)}
        if optimize:
            rec["optimize"] = True
        if coded is not None:
            rec.update({"scale": coded[j][0], "coded_height": coded[j][1][0], "coded_width": coded[j][1][1]})
        rec.update({"bytes": len(data), "bpp": 8 * len(data) / (H * W)})
        for k in FIELDS + (HVS_FIELDS if hvs else ()) + (FSIM_FIELDS if fsim else ()):
            rec[k] = None if m[k] is None else _json_number(m[k][j])
        for k, v in pm:
            rec[k] = None if v is None else float(v[0][j])
        rec["over_rate"] = bool(over)
        out.append(rec)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--originals", type=str, required=True, help="directory with the original images")
    ap.add_argument("--bitstreams", type=str, default=None, help="directory with *.c2df (decoded here unless --recon_dir is given)")
    ap.add_argument("--recon_dir", type=str, default=None, help="directory with reconstructions (decompress.py's results/)")
    ap.add_argument("--out", type=str, default=None, help="report file (JSON lines); default: stdout")
    ap.add_argument("--ckpt_path", type=str, default=None)
    ap.add_argument("--gpu_idx", type=int, default=0)
    ap.add_argument("--batch_size", type=int, default=32)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--anchor", choices=("jpeg",), default=None,
                    help="add a conventional codec at matched rate to every record: the largest JPEG quality in 1..95 whose file is "
                         "not larger than the container (needs --bitstreams for the sizes)")
    ap.add_argument("--anchor_subsampling", type=int, choices=(0, 1, 2), default=2, help="the anchor's chroma layout (Pillow's values)")
    ap.add_argument("--anchor_quality", type=int, default=None, help="fix the anchor's quality instead of searching (implies --anchor jpeg)")
    ap.add_argument("--anchor_optimize", action="store_true",
                    help="the anchor with Huffman tables fitted to every image, as Pillow's optimize=True (with --anchor jpeg or --anchor_quality)")
    ap.add_argument("--anchor_scales", type=int, nargs="+", default=None, metavar="R",
                    help="the anchor at reduced resolution: for every R (distinct integers in 1..16) the original is reduced to "
                         "ceil(H / R) x ceil(W / R) with Lanczos, coded, decoded and enlarged with bicubic; every image keeps the R "
                         "with the highest PSNR among those that fit its container (with --anchor_quality: exactly one R)")
    ap.add_argument("--lpips_ckpt", type=str, nargs="+", default=None,
                    help="state dict file(s) with the VGG16 trunk and the lin layers of LPIPS: adds \"lpips\" to every record")
    ap.add_argument("--lpips_alex_ckpt", type=str, nargs="+", default=None,
                    help="state dict file(s) with the AlexNet trunk and the lin layers of LPIPS: adds \"lpips_alex\" to every record")
    ap.add_argument("--dists_ckpt", type=str, nargs="+", default=None,
                    help="state dict file(s) with the VGG16 trunk and alpha, beta of DISTS: adds \"dists\" to every record")
    ap.add_argument("--fid_ckpt", type=str, nargs="+", default=None,
                    help="state dict file(s) of the Inception-v3 of FID: adds \"fid\", \"kid\", \"kid_std\" to the summary")
    ap.add_argument("--clip_ckpt", type=str, default=None,
                    help="state dict of the CLIP image tower (as compress.py --clip_ckpt): adds \"clip_sim\" to every record and the "
                         "retrieval figures clip_recall@k, clip_mrr, clip_median_rank to the summary")
    ap.add_argument("--niqe_params", type=str, default=None,
                    help="the pristine model of NIQE (.npz with mu_pris_param, cov_pris_param, or .mat): adds \"niqe\" and \"niqe_orig\" "
                         "to every record")
    ap.add_argument("--hvs", action="store_true",
                    help="add \"vifp\", \"gmsd\", \"psnr_hvs\" and \"psnr_hvs_m\" (luma measures that need no file) to every record")
    ap.add_argument("--fsim", action="store_true",
                    help="add \"fsim\" and \"fsimc\" (feature similarity on phase congruency, without and with chroma; no file needed) "
                         "to every record")
    ap.add_argument("--fid_patch", type=int, default=256,
                    help="side of the windows FID and KID are computed on (the HiFiC protocol); 0: whole images")
    args = ap.parse_args(argv)
    if not args.bitstreams and not args.recon_dir:
        ap.error("give --bitstreams, --recon_dir or both")
    if args.anchor_quality is not None and not 1 <= args.anchor_quality <= 100:
        ap.error("--anchor_quality must be in 1..100")
    if args.anchor and args.anchor_quality is None and not args.bitstreams:
        ap.error("--anchor jpeg matches the rate of the containers: give --bitstreams, or fix the quality with --anchor_quality")
    anchor = args.anchor or ("jpeg" if args.anchor_quality is not None else None)
    if args.anchor_optimize and not anchor:
        ap.error("--anchor_optimize changes the anchor: give --anchor jpeg or --anchor_quality")
    if args.anchor_scales is not None:
        if not anchor:
            ap.error("--anchor_scales changes the anchor: give --anchor jpeg or --anchor_quality")
        if any(not 1 <= r <= 16 for r in args.anchor_scales) or len(set(args.anchor_scales)) != len(args.anchor_scales):
            ap.error("--anchor_scales takes distinct integers in 1..16")
        if args.anchor_quality is not None and len(args.anchor_scales) != 1:
            ap.error("--anchor_quality fixes the quality: give exactly one scale with --anchor_scales")
        args.anchor_scales = sorted(args.anchor_scales)
    if args.batch_size < 1:
        ap.error("--batch_size must be at least 1")
    if args.fid_patch < 0:
        ap.error("--fid_patch must be 0 (whole images) or a window side")
    niqe_model = None
    if args.niqe_params:       # a bad file ends the command here, before any model is built
        from .niqe import Niqe
        try:
            niqe_model = Niqe(args.niqe_params)
        except (ValueError, OSError) as e:
            ap.error(f"--niqe_params: {e}")

    from concurrent.futures import ThreadPoolExecutor
    from . import quality

    torch.cuda.set_device(args.gpu_idx)
    dev = torch.device("cuda", args.gpu_idx)
    pair_metrics = []      # (key, model) of those asked for, in the order of PAIR_METRICS
    if args.lpips_ckpt:
        from .lpips import LpipsVGG
        pair_metrics.append(("lpips", LpipsVGG(args.lpips_ckpt, dev)))
    if args.lpips_alex_ckpt:
        from .lpips_alex import LpipsAlex
        pair_metrics.append(("lpips_alex", LpipsAlex(args.lpips_alex_ckpt, dev)))
    if args.dists_ckpt:
        from .dists import DistsVGG
        pair_metrics.append(("dists", DistsVGG(args.dists_ckpt, dev)))
    fid_sets = FidSets(args.fid_ckpt, args.fid_patch, dev) if args.fid_ckpt else None
    clip_sets = ClipSets(args.clip_ckpt, args.small, dev) if args.clip_ckpt else None
    originals = by_stem(glob(os.path.join(args.originals, "*.*")))
    containers = by_stem(glob(os.path.join(args.bitstreams, "*.c2df"))) if args.bitstreams else {}
    recons = by_stem(glob(os.path.join(args.recon_dir, "*.*"))) if args.recon_dir else None
    records = []

    def skip(name, reason):
        print(f"[SKIP] {name}: {reason}", file=sys.stderr)

    candidates = recons if recons is not None else containers
    for stem in sorted(set(originals) - set(candidates)):
        skip(stem, "no reconstruction for this original")
    for stem in sorted(set(candidates) - set(originals)):
        skip(stem, "no original for this reconstruction")
    stems = sorted(set(candidates) & set(originals))

    def measure_chunk(chunk, pending):
        """chunk: [(stem, reconstruction (H, W, 3) u8 on the device)]; pending: the loads of their originals, in the same order.
        Pairs of one size are measured as one batch."""
        groups = {}
        for (stem, rec), fut in zip(chunk, pending):
            org = fut.result()
            if isinstance(org, Exception):
                skip(stem, f"unreadable original ({org})")
            elif org.shape != tuple(rec.shape):
                skip(stem, f"original is {org.shape[0]}x{org.shape[1]}, reconstruction {rec.shape[0]}x{rec.shape[1]}")
            else:
                groups.setdefault(org.shape, []).append((stem, org, rec))
        for (H, W, _), members in groups.items():
            a = torch.from_numpy(np.stack([m[1] for m in members])).to(dev)
            b = torch.stack([m[2] for m in members])
            m = quality.measure(a, b)
            if args.hvs:
                m.update(quality.measure_hvs(a, b))
            if args.fsim:
                m.update(quality.measure_fsim(a, b))
            pm = [(k, model.measure(a, b)) for k, model in pair_metrics]
            sizes = [os.path.getsize(containers[stem]) if stem in containers else None for stem, _, _ in members]
            decoded = [] if fid_sets is not None or clip_sets is not None or niqe_model is not None else None
            anchors = jpeg_anchors(a, sizes, args.anchor_subsampling, args.anchor_quality, pair_metrics, decoded, args.anchor_optimize,
                                   args.anchor_scales, args.hvs, args.fsim) if anchor else None
            if clip_sets is not None:
                from .search import embedded_clip_codes
                ua, qa = clip_sets.embed(a)
                ub, _ = clip_sets.embed(b)
                sim = clip_sets.cosine(ua, ub)
                stored = clip_sets.stored_route_codes(a) if containers else None
                if anchor:
                    uj, _ = clip_sets.embed(decoded[0])
                    asim = clip_sets.cosine(ua, uj)
            if niqe_model is not None:
                nq_b, nq_a = niqe_model.measure(b), niqe_model.measure(a)
                nq_j = niqe_model.measure(decoded[0]) if anchor else None
            desc = fid_sets.windows(a) if fid_sets is not None else None
            if desc is not None:
                fid_sets.add("orig", a, desc)
                fid_sets.add("recon", b, desc)
                if anchor:
                    fid_sets.add("anchor", decoded[0], desc)
            for j, (stem, _, _) in enumerate(members):
                nbytes = sizes[j]
                rec = {"name": stem, "height": H, "width": W, "bytes": nbytes, "bpp": None if nbytes is None else 8 * nbytes / (H * W)}
                for k in FIELDS + (HVS_FIELDS if args.hvs else ()) + (FSIM_FIELDS if args.fsim else ()):
                    rec[k] = None if m[k] is None else _json_number(m[k][j])
                for k, v in pm:
                    rec[k] = None if v is None else float(v[0][j])
                if clip_sets is not None:
                    rec["clip_sim"] = float(sim[j])
                    clip_sets.codes[stem], clip_sets.units["recon"][stem] = qa[j], ub[j]
                    if containers:      # is --clip_ckpt the tower the archive was written with?
                        try:
                            rec["clip_code_match"] = bool(np.array_equal(embedded_clip_codes(containers[stem])[0], stored[j]))
                        except Exception:   # noqa: BLE001 -- no container for this image, or one without a code
                            rec["clip_code_match"] = None
                    if anchors:
                        over = anchors[j].pop("over_rate")
                        anchors[j]["clip_sim"] = float(asim[j])
                        anchors[j]["over_rate"] = over
                        clip_sets.units["anchor"][stem] = uj[j]
                if niqe_model is not None:
                    rec["niqe"] = None if np.isnan(nq_b[j]) else float(nq_b[j])
                    rec["niqe_orig"] = None if np.isnan(nq_a[j]) else float(nq_a[j])
                    if anchors:
                        over = anchors[j].pop("over_rate")
                        anchors[j]["niqe"] = None if np.isnan(nq_j[j]) else float(nq_j[j])
                        anchors[j]["over_rate"] = over
                if anchors:
                    rec["anchor"] = anchors[j]
                records.append(rec)

    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        if recons is not None:
            for s in range(0, len(stems), args.batch_size):
                part = stems[s:s + args.batch_size]
                pending = [pool.submit(load_rgb, originals[st]) for st in part]
                chunk = []
                keep = []
                for st, fut, arr in zip(part, pending, pool.map(load_rgb, [recons[st] for st in part])):
                    if isinstance(arr, Exception):
                        skip(st, f"unreadable reconstruction ({arr})")
                    else:
                        chunk.append((st, torch.from_numpy(arr).to(dev)))
                        keep.append(fut)
                measure_chunk(chunk, keep)
        else:
            from . import weights as W
            from .codec import Codec
            from .compress import load_state
            from .config import LARGE, SMALL
            from .filemaker import unpack_c2df
            cfg = SMALL if args.small else LARGE
            model = Codec(load_state(args.ckpt_path, W.full_spec, cfg, 1234), cfg, dev)
            model.hybrid_codec.quantize_feat.force_zero_thres = 0.12
            model.hybrid_codec.quantize_feat.update(force=True)
            items, groups = {}, {}
            for st in stems:
                try:
                    items[st] = unpack_c2df(containers[st])
                except Exception as e:   # noqa: BLE001 -- a truncated or foreign file
                    skip(st, f"unreadable container ({e})")
                    continue
                groups.setdefault(tuple(int(v) for v in items[st][0]["img_shape"]), []).append(st)
            for shape, members in groups.items():           # containers of one padded geometry decode as one batch (decompress.py)
                for s in range(0, len(members), args.batch_size):
                    part = members[s:s + args.batch_size]
                    pending = [pool.submit(load_rgb, originals[st]) for st in part]      # read underneath the GPU decode
                    x_hat = model.decode_batch([items[st][0] for st in part])
                    chunk = []
                    for j, st in enumerate(part):
                        pl, pr, pt, pb = items[st][1].get("padding", [0, 0, 0, 0])
                        H, Wd = x_hat.shape[2] - pt - pb, x_hat.shape[3] - pl - pr
                        chunk.append((st, to_u8_hwc_device(x_hat[j, :, pt:pt + H, pl:pl + Wd].clamp(-1, 1) * 0.5 + 0.5)))
                    measure_chunk(chunk, pending)

    records.sort(key=lambda r: r["name"])
    summary = json.dumps(summarise(records, fid_sets, clip_sets))
    lines = [json.dumps(r) for r in records]
    if args.out:
        with open(args.out, "w") as f:
            f.write("".join(ln + "\n" for ln in lines + [summary]))
    else:
        for ln in lines:
            print(ln)
    print(summary, file=sys.stderr)
    return 0 if records else 1


if __name__ == "__main__":
    sys.exit(main())
