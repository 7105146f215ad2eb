"""Streaming image ingest for the compress driver (replaces the reference's `Test_Dataset` + DataLoader,
compress.py:151-168,211-215, and its per-image `.to(device)` at :252).

The reference decodes one image per step into fp32 on 4 DataLoader workers.  At 300+ images/s per MI355X the host side
has to be a pipeline of its own, with bounded memory whatever the corpus size:

  1. header pass   -- `Image.open(path).size` reads the image header only (no pixel decode): every file of the shard
                      gets its geometry, and files of equal geometry are cut into batches.  File order inside a geometry
                      stays the sorted order.  With `pad_to` (the compress driver: 256) the geometry is the PADDED one, so
                      images of different sizes share a batch: the batch is a u8 canvas of its largest extents with every
                      image at the top left, and per-image extents travel with it (decode, padding and CLIP preprocessing
                      then work on each image's own extent; plan_batches caps such a batch at 4 x batch_size tiles).
  2. decode        -- JPEG batches (baseline Huffman files: what cameras and Pillow write) are decoded ON THE GPU: the thread
                      pool only reads the file bytes and parses markers (sgic_amd.jpeg), the compressed bytes cross PCIe
                      (~1/10 of the pixels) and csrc/jpeg.hip does Huffman decode, IDCT, chroma upsampling and colour
                      conversion, bit-exact with Pillow.  With `gpu_progressive` (SGIC_GPU_JPEG_PROGRESSIVE=1; off by
                      default) progressive JPEG batches, and batches mixing baseline and progressive files, are decoded
                      there too, scan by scan (sgic_amd.jpeg.ScanJpegBatch).  Other files (PNG, CMYK JPEG, ...) take the host
                      path: a thread pool (PIL releases the GIL while decoding) fills a PINNED u8 (B,H,W,3) buffer per
                      batch.  At most `depth` batches are prepared ahead of the consumer: memory is O(depth x batch), not
                      O(shard) -- a 10 k-image shard of 1024^2 inputs costs ~100 MB per in-flight batch, not 126 GB.
  3. H2D + convert -- the consumer copies the batch (compressed scans, or decoded u8: a quarter of the bytes of an fp32
                      copy) to the device asynchronously on a copy stream, the JPEG kernels run on that stream too (one
                      wave per image, small enough to sit beside a GEMM workgroup on the same CU), and one HIP kernel
                      does ToTensor, *2-1, NCHW and the replicate padding (ops.u8hwc_to_f32chw_pad).  Batch k+1 is
                      prepared under the GPU work of batch k.
"""
import os
import queue
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch


def image_size(path):
    """(H, W) from the file header; no pixel data is decoded"""
    from PIL import Image
    with Image.open(path) as im:
        w, h = im.size
    return h, w


def decode_rgb_u8(path, out_hw3):
    """`Image.open(path).convert('RGB')` (compress.py:160) decoded straight into a (H,W,3) u8 view"""
    from PIL import Image
    with Image.open(path) as im:
        a = np.asarray(im.convert("RGB"), dtype=np.uint8)
    if a.shape != tuple(out_hw3.shape):
        raise ValueError(f"{path}: decoded {a.shape}, header promised {tuple(out_hw3.shape)}")
    out_hw3[...] = a


def _read_bytes(path):
    with open(path, "rb") as f:
        return f.read()


def padded_size(h, w, pad_to):
    """(ceil(h / pad_to) * pad_to, ceil(w / pad_to) * pad_to): the geometry the encoder sees (get_padding_size)"""
    return -(-h // pad_to) * pad_to, -(-w // pad_to) * pad_to


def plan_batches(files, sizes, batch_size, pad_to=None, max_tiles=None):
    """-> list of (H, W, [indices into files]): one entry per batch; files of one geometry keep their order, geometries come in
    order of first appearance.  pad_to: group by the padded geometry (padded_size) instead of the exact size -- (H, W) is then that
    padded geometry -- and cut a batch before it holds more than max_tiles tiles of pad_to^2 (default 4 * batch_size, i.e.
    batch_size x 512^2 padded pixels; it never binds for images that pad to <= 512 x 512).  One image always makes a batch."""
    groups = {}
    for i, hw in enumerate(sizes):
        groups.setdefault(hw if pad_to is None else padded_size(hw[0], hw[1], pad_to), []).append(i)
    cap = 4 * batch_size if max_tiles is None else max_tiles
    plan = []
    for (h, w), idxs in groups.items():
        per = batch_size if pad_to is None else max(1, min(batch_size, cap // ((h // pad_to) * (w // pad_to))))
        for s in range(0, len(idxs), per):
            plan.append((h, w, idxs[s:s + per]))
    return plan


class Batch:
    """u8: pinned (B,H,W,3) host tensor (host-decoded batch), or None when `jpeg` holds a sgic_amd.jpeg.JpegBatch / ScanJpegBatch to
    decode on the GPU.  H x W: the batch's (canvas) geometry, the largest extents in it; hw: int32 (B, 2) extents of the images, each
    at the top left of the canvas (the canvas outside an image holds stale bytes); pad_hw: the padded geometry of a pad_to batch"""
    __slots__ = ("H", "W", "hw", "pad_hw", "indices", "paths", "u8", "jpeg", "_slot", "_owner")

    def release(self):
        """hand the pinned buffer back (call once the H2D copy of this batch has completed)"""
        if self._owner is not None:
            self._owner._free.put(self._slot)
            self._owner = None


class ShardLoader:
    """Iterate a shard as decoded, pinned u8 batches with a bounded read-ahead.

        for b in ShardLoader(files, 32):    # b.u8: pinned (B,H,W,3) uint8 tensor
            ...; b.release()
    A decode error is re-raised in the consumer at the position of the failing batch."""

    def __init__(self, files, batch_size=32, workers=None, depth=3, pin=True, gpu_jpeg=None, gpu_progressive=None, pad_to=None):
        """pad_to: batch images that pad to the same multiple of pad_to together (plan_batches); default: equal sizes only.
        gpu_jpeg: decode baseline JPEG batches on the GPU (default: when a GPU is present; SGIC_GPU_JPEG=0 turns it off).
        gpu_progressive: also decode the JPEG batches the baseline path refuses but the scan decoder takes (progressive and mixed
        baseline / progressive batches) on the GPU (default: off; SGIC_GPU_JPEG_PROGRESSIVE=1 turns it on); needs gpu_jpeg"""
        self.files = list(files)
        if gpu_jpeg is None:
            gpu_jpeg = torch.cuda.is_available() and os.environ.get("SGIC_GPU_JPEG", "1") != "0"
        if gpu_progressive is None:
            gpu_progressive = os.environ.get("SGIC_GPU_JPEG_PROGRESSIVE", "0") == "1"
        self.gpu_jpeg = bool(gpu_jpeg)
        self.gpu_progressive = self.gpu_jpeg and bool(gpu_progressive)
        self.gpu_batches = self.gpu_scan_batches = self.host_batches = 0
        self.batch_size, self.depth = int(batch_size), max(1, int(depth))
        self.workers = workers or min(16, max(2, (os.cpu_count() or 4)))
        self.pin = pin and torch.cuda.is_available()
        self._pool = ThreadPoolExecutor(max_workers=self.workers)
        self.sizes = list(self._pool.map(image_size, self.files))                 # header pass, no pixel decode
        self.pad_to = pad_to
        self.plan = plan_batches(self.files, self.sizes, self.batch_size, pad_to=pad_to)
        self._free = queue.Queue()
        for s in range(self.depth + 3):      # the consumer holds up to three batches (decoding ahead + GPU in flight + being written out)
            self._free.put(s)
        self._slots = {}
        self._q = queue.Queue(maxsize=self.depth)
        self._stop = False
        self._thread = threading.Thread(target=self._produce, name="sgic-ingest", daemon=True)
        self._thread.start()

    def __len__(self):
        return len(self.plan)

    def _buffer(self, slot, nbytes):
        """slot-owned flat pinned buffer, grown on demand; a batch views its first B*H*W*3 bytes"""
        t = self._slots.get(slot)
        if t is None or t.numel() < nbytes:
            # grown with headroom: pinning is a device-synchronising allocation, and compressed batches differ in size by a few percent
            nbytes = (int(nbytes * 1.5) + (1 << 20) - 1) & ~((1 << 20) - 1) if t is not None or self.gpu_jpeg else nbytes
            t = torch.empty(nbytes, dtype=torch.uint8)
            if self.pin:
                t = t.pin_memory()
            self._slots[slot] = t
        return t

    def _produce(self):
        try:
            for (h, w, idxs) in self.plan:
                while True:                      # wait for a free pinned slot (bounded memory), but notice close()
                    if self._stop:
                        return
                    try:
                        slot = self._free.get(timeout=0.1)
                        break
                    except queue.Empty:
                        continue
                n = len(idxs)
                hw = np.array([self.sizes[i] for i in idxs], dtype=np.int32).reshape(n, 2)
                b = Batch()
                b.indices, b.paths, b.jpeg, b.hw = idxs, [self.files[i] for i in idxs], None, hw
                if self.pad_to:      # the canvas: the largest extents of the batch
                    b.H, b.W, b.pad_hw = int(hw[:, 0].max()), int(hw[:, 1].max()), (h, w)
                else:
                    b.H, b.W, b.pad_hw = h, w, None
                canvas = (b.H, b.W) if self.pad_to else None
                scans = False
                if self.gpu_jpeg and all(p.lower().endswith((".jpg", ".jpeg")) for p in b.paths):
                    from . import jpeg as J
                    alloc = lambda nbytes: self._buffer(slot, nbytes)     # the slot's pinned buffer: read in place by the kernels
                    datas = None
                    try:     # file bytes + marker parsing on the pool; the pixels never exist on the host
                        datas = list(self._pool.map(_read_bytes, b.paths))
                        b.jpeg = J.JpegBatch(datas, pool=self._pool, alloc=alloc, canvas=canvas)
                    except Exception:      # noqa: BLE001 -- J.Unsupported (progressive / CMYK / ...) or a file the parser chokes on:
                        b.jpeg = None      # this batch takes the host decoder, which raises a proper error for a really broken file
                    if b.jpeg is None and datas is not None and self.gpu_progressive:
                        try:     # progressive / mixed batch: decoded scan by scan
                            b.jpeg, scans = J.ScanJpegBatch(datas, pool=self._pool, alloc=alloc, canvas=canvas), True
                        except Exception:  # noqa: BLE001 -- as above: the host decoder takes it
                            b.jpeg = None
                    if b.jpeg is not None and not np.array_equal(b.jpeg.hw, hw):     # a parsed size differs from its header pass
                        b.jpeg = None
                if b.jpeg is not None:
                    b.u8, b._slot, b._owner = None, slot, self     # the slot returns with release(), after the copy has completed
                    if scans:
                        self.gpu_scan_batches += 1
                    else:
                        self.gpu_batches += 1
                else:
                    ch, cw = b.H, b.W
                    flat = self._buffer(slot, n * ch * cw * 3)
                    u8 = flat[:n * ch * cw * 3].view(n, ch, cw, 3)
                    arr = u8.numpy()
                    list(self._pool.map(lambda j: decode_rgb_u8(self.files[idxs[j]], arr[j, :hw[j, 0], :hw[j, 1]]), range(n)))
                    b.u8, b._slot, b._owner = u8, slot, self
                    self.host_batches += 1
                self._q.put(b)
            self._q.put(None)
        except BaseException as e:               # surfaces in the consumer
            self._q.put(e)

    def __iter__(self):
        while True:
            item = self._q.get()
            if item is None:
                return
            if isinstance(item, BaseException):
                raise item
            yield item

    def close(self):
        self._stop = True
        try:
            while True:
                self._q.get_nowait()
        except queue.Empty:
            pass
        self._thread.join(timeout=5)
        self._pool.shutdown(wait=False)


class DeviceIngest:
    """batch -> padded fp32 NCHW on the device.  Two steps so that a driver can run one batch ahead:
        tok = start(batch)        enqueue, on the copy stream, the GPU JPEG decode (compressed bytes are read in place from pinned host
                                  memory) or the async H2D copy of a host-decoded u8 batch; returns at once
        x, done = finish(tok, pad)  on the launch stream: wait for `tok`, then the fused ToTensor / *2-1 / NCHW / replicate-pad kernel
    ORDER MATTERS: HIP streams can share a hardware queue, where packets launch in enqueue order -- a decode enqueued behind the ~750
    kernels of a batch starts when that batch ends (measured: a 10 ms bubble per batch), one enqueued BEFORE them runs under them.
    compress.py therefore calls start(batch k+1) before it submits batch k.  __call__ = start + finish."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.copy_stream = torch.cuda.Stream(device=self.device)

    def start(self, batch):
        with torch.cuda.stream(self.copy_stream):
            if batch.jpeg is not None:
                d = batch.jpeg.decode(self.device, check=False)
                # the per-image error codes come back on THIS stream into the pinned staging buffer, ahead of `done`: the consumer
                # reads them on the host after done.synchronize() -- a .cpu() on the launch stream would queue behind the next
                # batch's kernels and stall the pipeline for a whole batch
                batch.jpeg.err_host.copy_(batch.jpeg.last_err, non_blocking=True)
            else:
                d = torch.empty(batch.u8.shape, dtype=torch.uint8, device=self.device)
                d.copy_(batch.u8, non_blocking=True)
            done = torch.cuda.Event()
            done.record()
        return d, done

    def finish(self, tok, pad, hw=None):
        """pad = (pl, pr, pt, pb) of compress.py:258-261 -> x (B,3,H+pt+pb,W+pl+pr) fp32 in [-1,1] on the launch stream.
        hw: the (B, 2) extents of a canvas batch whose images differ in size (Batch.hw); every image is then padded from its OWN
        right / bottom edge, `pad` being the canvas's padding (right / bottom only)"""
        from . import ops
        d, done = tok
        cur = torch.cuda.current_stream()
        cur.wait_event(done)
        d.record_stream(cur)
        if hw is not None:
            pl, pr, pt, pb = pad
            if pl or pt:
                raise ValueError("a batch of images of different sizes is padded on the right and bottom only")
            x = ops.u8canvas_to_f32chw_pad(d, hw, d.shape[1] + pb, d.shape[2] + pr)
        else:
            x = ops.u8hwc_to_f32chw_pad(d, *pad)
        return x, done

    def __call__(self, batch, pad, hw=None):
        return self.finish(self.start(batch), pad, hw)
