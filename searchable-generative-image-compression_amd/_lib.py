"""ctypes binding of libsgic.so (C ABI in include/sgic.h).  Fails loudly: no library -> ImportError,
no GPU -> RuntimeError at the first op.  There is deliberately no CPU fallback."""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.environ.get("SGIC_LIB") or os.path.join(_HERE, "libsgic.so")   # SGIC_LIB: A/B builds of the library (tools)

if not os.path.exists(_SO):
    raise ImportError(f"{_SO} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                      "(hipcc --offload-arch=gfx950). The product path has no CPU fallback.")

lib = C.CDLL(_SO)
lib.sgic_last_error.restype = C.c_char_p
lib.sgic_pack12_size.restype = C.c_size_t
lib.sgic_pack12_size.argtypes = [C.c_size_t]

c_void_p, c_int, c_float, c_size_t = C.c_void_p, C.c_int, C.c_float, C.c_size_t
# sgic_quality_u8 (csrc/quality.hip): (d_a, d_b, B, H, W, d_work, work_bytes, d_sse, d_levels, stream)
lib.sgic_quality_u8_work_bytes.argtypes = [c_int, c_int, c_int, C.POINTER(c_size_t)]
lib.sgic_quality_u8.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p]
# sgic_niqe_u8 (csrc/niqe.hip): (d_img, B, H, W, h_weights, d_work, work_bytes, d_stats, d_sharp, stream)
lib.sgic_niqe_u8_work_bytes.argtypes = [c_int, c_int, c_int, C.POINTER(c_size_t)]
lib.sgic_niqe_u8.argtypes = [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p]
# csrc/hvs.hip: sgic_hvs_luma_u8 (d_img, B, H, W, d_y, stream); sgic_hvs_{vifp,gmsd} (d_ya, d_yb, B, H, W, d_work, work_bytes, d_out,
# stream); sgic_hvs_psnr the same with h_q in front of d_work
lib.sgic_hvs_luma_u8.argtypes = [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]
for _m in ("vifp", "gmsd", "psnr"):
    getattr(lib, f"sgic_hvs_{_m}_work_bytes").argtypes = [c_int, c_int, c_int, C.POINTER(c_size_t)]
lib.sgic_hvs_vifp.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p, c_void_p]
lib.sgic_hvs_gmsd.argtypes = lib.sgic_hvs_vifp.argtypes
lib.sgic_hvs_psnr.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]
# csrc/fsim.hip: sgic_fsim_planes_u8 (d_img, B, H, W, d_out, stream); sgic_fsim_phasecong (d_planes, B, h, w, d_work, work_bytes, d_pc,
# stream); sgic_fsim (d_a, d_b, B, H, W, d_work, work_bytes, d_fsim, d_fsimc, stream)
lib.sgic_fsim_planes_u8.argtypes = [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]
lib.sgic_fsim_phasecong_work_bytes.argtypes = [c_int, c_int, c_int, C.POINTER(c_size_t)]
lib.sgic_fsim_work_bytes.argtypes = [c_int, c_int, c_int, C.POINTER(c_size_t)]
lib.sgic_fsim_phasecong.argtypes = [c_void_p, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p, c_void_p]
lib.sgic_fsim.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p]
# sgic_jpeg_encode_batch (csrc/jpeg_enc.hip): (d_rgb, B, H, W, subsampling, h_qt, d_work, work_bytes, d_out, cap, d_len, d_err, stream)
lib.sgic_jpeg_encode_cap.argtypes = [c_int, c_int, c_int, C.POINTER(c_size_t)]
lib.sgic_jpeg_encode_work_bytes.argtypes = [c_int, c_int, c_int, c_int, C.POINTER(c_size_t)]
lib.sgic_jpeg_encode_batch.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p, c_size_t, c_void_p,
                                       c_void_p, c_void_p]
# sgic_jpeg_encode_opt_batch: the same with (d_huff, d_nval) in front of the stream
lib.sgic_jpeg_encode_opt_cap.argtypes = lib.sgic_jpeg_encode_cap.argtypes
lib.sgic_jpeg_encode_opt_work_bytes.argtypes = lib.sgic_jpeg_encode_work_bytes.argtypes
lib.sgic_jpeg_encode_opt_batch.argtypes = lib.sgic_jpeg_encode_batch.argtypes[:-1] + [c_void_p, c_void_p, c_void_p]
# sgic_jpeg_encode_prog_batch: the optimised call's arguments, the outputs widened to ten scans
lib.sgic_jpeg_encode_prog_cap.argtypes = lib.sgic_jpeg_encode_cap.argtypes
lib.sgic_jpeg_encode_prog_work_bytes.argtypes = lib.sgic_jpeg_encode_work_bytes.argtypes
lib.sgic_jpeg_encode_prog_batch.argtypes = lib.sgic_jpeg_encode_opt_batch.argtypes
# sgic_lpips_head (csrc/lpips.hip): (d_feat, d_w, B, H, W, C, d_work, work_bytes, d_d, stream)
lib.sgic_lpips_head_work_bytes.argtypes = [c_int, c_int, c_int, C.POINTER(c_size_t)]
lib.sgic_lpips_head.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p, c_void_p]
# sgic_dists_moments (csrc/dists.hip): (d_feat, B, H, W, C, d_work, work_bytes, d_sums, stream)
lib.sgic_dists_moments_work_bytes.argtypes = [c_int, c_int, c_int, c_int, C.POINTER(c_size_t)]
lib.sgic_dists_moments.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p, c_void_p]
# sgic_resize_u8_batch (csrc/resize.hip): (d_in, B, H, W, d_out, OH, OW, filter, d_work, work_bytes, stream)
lib.sgic_resize_u8_work_bytes.restype = c_size_t
lib.sgic_resize_u8_work_bytes.argtypes = [c_int] * 6
lib.sgic_resize_u8_coeffs.argtypes = [c_int, c_int, c_int, c_int, c_void_p, c_void_p]
lib.sgic_resize_u8_batch.argtypes = [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p]


class LaunchOpts(C.Structure):
    """sgic_launch_opts (include/sgic.h): per-call launch options of the GEMM-family / attention entry points"""
    _fields_ = [("tile_mode", C.c_int), ("attn_mode", C.c_int), ("profiler", C.c_void_p), ("w_packed", C.c_int), ("a_packed", C.c_int)]


def launch_opts(tile_mode=0, attn_mode=0, profiler=None, w_packed=0, a_packed=0):
    """-> a by-reference ctypes argument, or NULL when every field is at its default"""
    if not tile_mode and not attn_mode and not profiler and not w_packed and not a_packed:
        return c_void_p(0)
    return C.byref(LaunchOpts(int(tile_mode), int(attn_mode), profiler, int(w_packed), int(a_packed)))


class SgicError(RuntimeError):
    pass


def check(rc, what=""):
    if rc != 0:
        raise SgicError(f"libsgic {what} failed rc={rc}: {lib.sgic_last_error().decode()}")


def require_gpu():
    if not torch.cuda.is_available():
        raise RuntimeError("sgic_amd needs an MI355X (gfx950) GPU: the hot path is HIP-only, no CPU fallback")


try:   # the raw HIP stream of torch's current stream without building a Stream object (8 us -> 0.3 us per launch)
    _raw_stream = torch._C._cuda_getCurrentRawStream
    _get_device = torch._C._cuda_getDevice
except AttributeError:   # a torch without the private hooks
    _raw_stream = None


def stream():
    """HIP stream of torch's CURRENT stream on the current device (honours `with torch.cuda.stream(...)`)"""
    if _raw_stream is not None:
        return c_void_p(_raw_stream(_get_device()))
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    """device (or host) pointer of a contiguous tensor / numpy array; None -> NULL"""
    if t is None:
        return c_void_p(0)
    if isinstance(t, torch.Tensor):
        assert t.is_contiguous(), "sgic kernels take contiguous tensors"
        return c_void_p(t.data_ptr())
    return c_void_p(t.ctypes.data)


_NO_STREAM = {"sgic_pmf_to_quantized_cdf", "sgic_cdf_table_create", "sgic_profiler_create", "sgic_profiler_begin", "sgic_profiler_end",
              "sgic_clip_preprocess_ragged_workspace", "sgic_clip_preprocess_u8canvas_workspace", "sgic_search_codes_u8_work_bytes",
              "sgic_search_codes_f32q_work_bytes", "sgic_search_rank_work_bytes", "sgic_assign_codes_f32c_work_bytes", "sgic_quality_u8_work_bytes", "sgic_jpeg_encode_cap",
              "sgic_jpeg_encode_work_bytes", "sgic_jpeg_encode_opt_cap", "sgic_jpeg_encode_opt_work_bytes", "sgic_jpeg_encode_prog_cap",
              "sgic_jpeg_encode_prog_work_bytes", "sgic_lpips_head_work_bytes", "sgic_dists_moments_work_bytes",
              "sgic_niqe_u8_work_bytes", "sgic_resize_u8_coeffs", "sgic_hvs_vifp_work_bytes", "sgic_hvs_gmsd_work_bytes",
              "sgic_hvs_psnr_work_bytes", "sgic_fsim_work_bytes", "sgic_fsim_phasecong_work_bytes"}


def call(name, *args):
    """call lib.<name>(*args, current HIP stream) -> check return code.  Every device entry point of
    the C ABI takes the stream as its LAST argument; it is appended here."""
    fn = getattr(lib, name)
    conv = []
    for a in args:
        if isinstance(a, (torch.Tensor,)) or a is None or hasattr(a, "ctypes"):
            conv.append(ptr(a))
        elif isinstance(a, bool):
            conv.append(c_int(int(a)))
        elif isinstance(a, int):
            conv.append(c_int(a))
        elif isinstance(a, float):
            conv.append(c_float(a))
        else:
            conv.append(a)
    if name not in _NO_STREAM:
        conv.append(stream())
    check(fn(*conv), name)
