"""Streaming image ingest for the compress driver (replaces the reference's `Test_Dataset` + DataLoader,
compress.py:151-168,211-215, and its per-image `.to(device)` at :252).

The reference decodes one image per step into fp32 on 4 DataLoader workers.  At 300+ images/s per MI355X the host side
has to be a pipeline of its own, with bounded memory whatever the corpus size:

  1. header pass   -- `Image.open(path).size` reads the image header only (no pixel decode): every file of the shard
                      gets its geometry, and consecutive files of equal geometry are cut into batches (a batch shares
                      padding and CLIP resize geometry).  File order inside a geometry stays the sorted order.
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


def plan_batches(files, sizes, batch_size):
    """-> list of (H, W, [indices into files]): one entry per batch; files of one geometry keep their order"""
    groups = {}
    for i, hw in enumerate(sizes):
        groups.setdefault(hw, []).append(i)
    plan = []
    for (h, w), idxs in groups.items():
        for s in range(0, len(idxs), batch_size):
            plan.append((h, w, idxs[s:s + batch_size]))
    return plan


class Batch:
    """u8: pinned (B,H,W,3) host tensor (host-decoded batch), or None when `jpeg` holds a sgic_amd.jpeg.JpegBatch / ScanJpegBatch to
    decode on the GPU"""
    __slots__ = ("H", "W", "indices", "paths", "u8", "jpeg", "_slot", "_owner")

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

    def __init__(self, files, batch_size=32, workers=None, depth=3, pin=True, gpu_jpeg=None, gpu_progressive=None):
        """gpu_jpeg: decode baseline JPEG batches on the GPU (default: when a GPU is present; SGIC_GPU_JPEG=0 turns it off).
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
        self.plan = plan_batches(self.files, self.sizes, self.batch_size)
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
                b = Batch()
                b.H, b.W, b.indices, b.paths, b.jpeg = h, w, idxs, [self.files[i] for i in idxs], None
                scans = False
                if self.gpu_jpeg and all(p.lower().endswith((".jpg", ".jpeg")) for p in b.paths):
                    from . import jpeg as J
                    alloc = lambda nbytes: self._buffer(slot, nbytes)     # the slot's pinned buffer: read in place by the kernels
                    datas = None
                    try:     # file bytes + marker parsing on the pool; the pixels never exist on the host
                        datas = list(self._pool.map(_read_bytes, b.paths))
                        b.jpeg = J.JpegBatch(datas, pool=self._pool, alloc=alloc)
                    except Exception:      # noqa: BLE001 -- J.Unsupported (progressive / CMYK / ...) or a file the parser chokes on:
                        b.jpeg = None      # this batch takes the host decoder, which raises a proper error for a really broken file
                    if b.jpeg is None and datas is not None and self.gpu_progressive:
                        try:     # progressive / mixed batch: decoded scan by scan
                            b.jpeg, scans = J.ScanJpegBatch(datas, pool=self._pool, alloc=alloc), True
                        except Exception:  # noqa: BLE001 -- as above: the host decoder takes it
                            b.jpeg = None
                    if b.jpeg is not None and (b.jpeg.H, b.jpeg.W) != (h, w):
                        b.jpeg = None
                if b.jpeg is not None:
                    b.u8, b._slot, b._owner = None, slot, self     # the slot returns with release(), after the copy has completed
                    if scans:
                        self.gpu_scan_batches += 1
                    else:
                        self.gpu_batches += 1
                else:
                    flat = self._buffer(slot, n * h * w * 3)
                    u8 = flat[:n * h * w * 3].view(n, h, w, 3)
                    arr = u8.numpy()
                    list(self._pool.map(lambda j: decode_rgb_u8(self.files[idxs[j]], arr[j]), range(n)))
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

    def finish(self, tok, pad):
        """pad = (pl, pr, pt, pb) of compress.py:258-261 -> x (B,3,Hp,Wp) fp32 in [-1,1] on the launch stream"""
        from . import ops
        d, done = tok
        cur = torch.cuda.current_stream()
        cur.wait_event(done)
        d.record_stream(cur)
        x = ops.u8hwc_to_f32chw_pad(d, *pad)
        return x, done

    def __call__(self, batch, pad):
        return self.finish(self.start(batch), pad)
