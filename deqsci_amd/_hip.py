"""ctypes binding of the C-ABI HIP library (include/deqsci_hip.h -> lib/libdeqsci_hip.so).

PyTorch is used for device memory and streams only: every function takes torch CUDA(HIP)
tensors, passes raw device pointers + the current HIP stream to the library and returns
torch tensors.  There is NO CPU fallback: a missing library or a non-GPU tensor raises.
"""
import ctypes
import math
import os

import torch

LAYOUT_HWB = 0   # (bsz,H,W,B)  reference API layout
LAYOUT_BHW = 1   # (bsz,B,H,W)  planar / denoiser layout
MAX_M = 8
PART_STRIDE = MAX_M + 1
BN_TRAIN_CHUNK, BN_TRAIN_MAX_WG = 128, 1024   # DEQSCI_BN_TRAIN_CHUNK, DEQSCI_BN_TRAIN_MAX_WG: the pixels of a workgroup of csrc/bn_train.hip, its most workgroups
WGRAD_CHAIN = 4096   # DEQSCI_WGRAD_CHAIN: the most products a weight-gradient entry sums in fp32 before the float64 stage

# DEQSCI_HIP_LIB: another build of the SAME library (tools only: the -DDEQSCI_DIAG variant of `make diag`, a stamp build of tools/lib_variants.sh)
_LIB_PATH = os.environ.get("DEQSCI_HIP_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libdeqsci_hip.so")
_lib = None

_i64, _int, _f32, _ptr = ctypes.c_int64, ctypes.c_int, ctypes.c_float, ctypes.c_void_p
_f64 = ctypes.c_double
_u64 = ctypes.c_uint64

# name -> argtypes; the single source of truth for tests/test_cabi_exports.py too
SIGNATURES = {
    "deqsci_sci_forward_f32": [_ptr, _ptr, _ptr, _i64, _i64, _i64, _i64, _int, _int, _ptr],
    "deqsci_sci_adjoint_f32": [_ptr, _ptr, _ptr, _i64, _i64, _i64, _i64, _int, _int, _ptr],
    "deqsci_phi_sum_f32": [_ptr, _ptr, _i64, _i64, _i64, _i64, _int, _ptr],
    "deqsci_gap_update_f32": [_ptr, _ptr, _ptr, _ptr, _ptr, _i64, _i64, _i64, _i64, _int, _int, _int, _ptr],
    "deqsci_gap_update_grad_f32": [_ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _i64, _i64, _i64, _i64, _int, _int, _ptr],
    "deqsci_sci_mask_grad_f32": [_ptr, _ptr, _ptr, _i64, _i64, _i64, _i64, _int, _int, _ptr],
    "deqsci_phi_sum_grad_f32": [_ptr, _ptr, _ptr, _i64, _i64, _i64, _i64, _int, _ptr],
    "deqsci_transpose_f32": [_ptr, _ptr, _i64, _i64, _i64, _i64, _int, _ptr],
    "deqsci_residual_out_f32": [_ptr, _ptr, _ptr, _i64, _i64, _i64, _i64, _int, _ptr],
    "deqsci_residual_store_f32": [_ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _i64, _i64, _int, _int, _int, _ptr],
    "deqsci_anderson_solve_f32": [_ptr, _ptr, _ptr, _ptr, _i64, _i64, _int, _int, _int, _int, _f32, _f32, _ptr],
    "deqsci_anderson_solve_gram_f32": [_ptr, _ptr, _ptr, _ptr, _i64, _i64, _int, _int, _int, _int, _f32, _f32, _ptr, _ptr],
    "deqsci_anderson_solve_ref_f32": [_ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _i64, _i64, _int, _int, _int, _int, _f32, _f32, _ptr],
    "deqsci_residual_store_ref_f32": [_ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _i64, _i64, _int, _int, _int, _ptr],
    "deqsci_anderson_apply_solve_ref_f32": [_ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _i64, _i64, _int, _int, _int, _int, _f32, _f32, _ptr],
    "deqsci_gram_ref_fusable": [_i64, _i64],
    "deqsci_gram_row_chain16_f32": [_ptr, _ptr, _ptr, _i64, _i64, _int, _int, _int, _int, _ptr],
    "deqsci_anderson_mix_f32": [_ptr, _ptr, _ptr, _ptr, _f32, _int, _i64, _i64, _int, _ptr],
    "deqsci_anderson_mix_gap_f32": [_ptr, _ptr, _ptr, _f32, _int, _int, _ptr, _ptr, _ptr, _ptr, _ptr,
                                    _i64, _i64, _i64, _i64, _int, _int, _ptr],
    "deqsci_anderson_mix_gap_timed_f32": [_ptr, _ptr, _ptr, _f32, _int, _int, _ptr, _ptr, _ptr, _ptr, _ptr,
                                          _i64, _i64, _i64, _i64, _int, _int, _ptr, _ptr, _ptr],
    "deqsci_bias_relu_f32": [_ptr, _ptr, _i64, _i64, _i64, _int, _int, _ptr],
    "deqsci_ffdnet_tail_f32": [_ptr, _ptr, _ptr, _ptr, _i64, _i64, _i64, _ptr],
    "deqsci_ffdnet_head_f32": [_ptr, _ptr, _ptr, _i64, _ptr, _i64, _i64, _i64, _ptr],
    "deqsci_conv3x3_c64_to_1_f32": [_ptr, _ptr, _ptr, _ptr, _i64, _i64, _i64, _ptr],
    "deqsci_conv3x3_c1_to_64_f32": [_ptr, _ptr, _ptr, _i64, _i64, _i64, _int, _ptr],
    "deqsci_conv3x3_c64_winograd_f32": [_ptr, _ptr, _ptr, _ptr, _i64, _i64, _i64, _int, _ptr],
    "deqsci_conv3x3_c64_winograd_timed_f32": [_ptr, _ptr, _ptr, _ptr, _i64, _i64, _i64, _int, _ptr, _ptr, _ptr],
    "deqsci_conv3x3_c64_winograd44_f32": [_ptr, _ptr, _ptr, _ptr, _i64, _i64, _i64, _int, _ptr],
    "deqsci_conv3x3_c64_winograd44_timed_f32": [_ptr, _ptr, _ptr, _ptr, _i64, _i64, _i64, _int, _ptr, _ptr, _ptr],
    "deqsci_conv3x3_c64_winograd44_layout_f32": [_ptr, _ptr, _ptr, _ptr, _i64, _i64, _i64, _int, _int, _int, _ptr, _ptr, _ptr],
    "deqsci_conv3x3_c64_split16": [_ptr, _ptr, _ptr, _ptr, _i64, _i64, _i64, _int, _int, _ptr, _int, _ptr, _int, _ptr, _int, _ptr, _ptr, _ptr],
    "deqsci_conv3x3_c64_split16_stack": [_ptr, _ptr, _ptr, _ptr, _int, _i64, _i64, _i64, _ptr, _i64, _int, _int, _ptr, _ptr, _ptr, _ptr],
    "deqsci_conv3x3_c64_wino16": [_ptr, _ptr, _ptr, _ptr, _i64, _i64, _i64, _int, _int, _ptr, _int, _ptr, _int, _ptr, _ptr, _ptr],
    "deqsci_conv3x3_c64_wino16_stack": [_ptr, _ptr, _ptr, _ptr, _int, _i64, _i64, _i64, _ptr, _i64, _int, _int, _ptr, _ptr, _ptr, _ptr],
    "deqsci_f32_to_split16": [_ptr, _ptr, _i64, _i64, _i64, _ptr, _int, _ptr],
    "deqsci_absmax_f32": [_ptr, _i64, _i64, _ptr, _ptr],
    "deqsci_ffdnet_tail_split16": [_ptr, _ptr, _ptr, _i64, _i64, _i64, _int, _ptr, _int, _ptr],
    "deqsci_ffdnet_head_split16": [_ptr, _ptr, _ptr, _i64, _ptr, _i64, _i64, _i64, _int, _ptr, _int, _ptr, _int, _ptr, _ptr],
    "deqsci_conv3x3_c64_to_1_split16": [_ptr, _ptr, _ptr, _i64, _i64, _i64, _int, _ptr, _int, _ptr],
    "deqsci_conv3x3_c64_to_1_p32": [_ptr, _ptr, _ptr, _i64, _i64, _i64, _int, _ptr, _int, _ptr],
    "deqsci_conv3x3_c1_to_64_p32": [_ptr, _ptr, _ptr, _i64, _i64, _i64, _int, _ptr, _int, _ptr, _ptr],
    "deqsci_ffdnet_head_p32": [_ptr, _ptr, _ptr, _i64, _ptr, _i64, _i64, _i64, _int, _ptr, _int, _ptr, _int, _ptr],
    "deqsci_ffdnet_tail_p32": [_ptr, _ptr, _ptr, _i64, _i64, _i64, _int, _ptr, _int, _ptr],
    "deqsci_conv3x3_c1_to_64_sp16": [_ptr, _ptr, _ptr, _i64, _i64, _i64, _int, _ptr, _int, _ptr, _ptr],
    "deqsci_ssim_f32": [_ptr, _ptr, _ptr, _i64, _i64, _i64, _i64, _int, _int, _int, _int, _ptr, _ptr],
    "deqsci_sqerr_rows_f32": [_ptr, _ptr, _ptr, _i64, _i64, _i64, _int, _ptr, _ptr],
    "deqsci_gaptv_f32": [_ptr, _ptr, _ptr, _ptr, _i64, _i64, _i64, _i64, _int, _int, _f64, _f64, _f64, _int, _ptr, _ptr, _ptr],
    "deqsci_tv_chambolle_f32": [_ptr, _ptr, _i64, _i64, _i64, _f64, _f64, _int, _f64, _ptr, _ptr, _ptr],
    "deqsci_relu_mask_pack_f32": [_ptr, _ptr, _i64, _ptr],
    "deqsci_conv3x3_c64_winograd_masked_f32": [_ptr, _ptr, _ptr, _ptr, _i64, _i64, _i64, _ptr],
    "deqsci_conv3x3_c1_to_64_masked_f32": [_ptr, _ptr, _ptr, _ptr, _i64, _i64, _i64, _ptr],
    "deqsci_ffdnet_head_masked_f32": [_ptr, _ptr, _ptr, _ptr, _i64, _i64, _i64, _ptr],
    "deqsci_power_step_f32": [_ptr, _ptr, _ptr, _ptr, _i64, _i64, _ptr, _ptr],
    "deqsci_broyden_dots_f32": [_ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _i64, _i64, _int, _int, _ptr],
    "deqsci_broyden_update_f32": [_ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _i64, _i64, _int, _int, _int, _ptr],
    "deqsci_epsilon2_norms_f32": [_ptr, _ptr, _ptr, _ptr, _ptr, _i64, _i64, _ptr],
    "deqsci_epsilon2_update_f32": [_ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _i64, _i64, _f32, _ptr],
    "deqsci_wgrad3x3_c64_c64_f32": [_ptr, _ptr, _ptr, _i64, _i64, _i64, _ptr, _ptr],
    "deqsci_wgrad3x3_c1_c64_f32": [_ptr, _ptr, _ptr, _int, _i64, _i64, _i64, _ptr, _ptr],
    "deqsci_wgrad3x3_c64_c64_bn_f32": [_ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _i64, _i64, _i64, _ptr, _ptr],
    "deqsci_wgrad3x3_shuffle_f32": [_ptr, _ptr, _i64, _ptr, _ptr, _int, _i64, _i64, _i64, _ptr, _ptr],
    "deqsci_realsn_power_f32": [_ptr, _ptr, _ptr, _ptr, _ptr, _int, _f32, _f32, _i64, _i64, _i64, _i64, _ptr, _ptr],
    "deqsci_realsn_grad_f32": [_ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _f32, _i64, _i64, _i64, _i64, _ptr, _ptr],
    "deqsci_realsn_pack_f32": [_ptr, _ptr, _ptr, _ptr, _i64, _i64, _ptr],
    "deqsci_bn_train_stats_f32": [_ptr, _ptr, _ptr, _ptr, _ptr, _f64, _i64, _ptr, _ptr],
    "deqsci_bn_train_apply_f32": [_ptr, _ptr, _ptr, _ptr, _f64, _ptr, _ptr, _int, _i64, _ptr],
    "deqsci_bn_train_grad_stats_f32": [_ptr, _ptr, _ptr, _f64, _ptr, _ptr, _ptr, _i64, _ptr, _ptr],
    "deqsci_bn_train_grad_apply_f32": [_ptr, _ptr, _ptr, _ptr, _ptr, _f64, _ptr, _i64, _ptr],
    "deqsci_mse_stats_grad_f32": [_ptr, _ptr, _ptr, _ptr, _i64, _f32, _ptr, _ptr],
    "deqsci_adam_step_f32": [_ptr, _int, _f32, _f32, _f32, _f32, _f32, _ptr],
    "deqsci_adam_step_clipped_f32": [_ptr, _int, _f32, _f32, _f32, _f32, _f32, _ptr, _ptr],
    "deqsci_grad_norm_f32": [_ptr, _i64, _f64, _ptr, _ptr, _ptr],
    "deqsci_grad_scale_f32": [_ptr, _i64, _ptr, _ptr],
    "deqsci_synth_batch_u8": [_ptr, _i64, _ptr, _i64, _ptr, _i64, _ptr, _ptr, _i64, _i64, _i64, _ptr],
    "deqsci_rgb_to_gray_u8": [_ptr, _ptr, _i64, _ptr],
    "deqsci_philox_words_u32": [_ptr, _ptr, _i64, _i64, _u64, _ptr],
    "deqsci_philox_normal_f32": [_ptr, _ptr, _i64, _i64, _u64, _ptr],
    "deqsci_sensor_noise_f32": [_ptr, _ptr, _ptr, _i64, _i64, _u64, _f32, _f32, _int, _f32, _ptr],
    "deqsci_event_create": [ctypes.POINTER(_ptr)],
    "deqsci_event_destroy": [_ptr],
    "deqsci_event_elapsed_ms": [_ptr, _ptr, ctypes.POINTER(_f32)],
}
OTHER_EXPORTS = ("deqsci_version", "deqsci_error_string", "deqsci_anderson_chunks",
                 "deqsci_partials_bytes", "deqsci_gram_bytes", "deqsci_gram_ref_bytes", "deqsci_ssim_workspace_bytes",
                 "deqsci_gaptv_workspace_bytes", "deqsci_tv_chambolle_workspace_bytes", "deqsci_sqerr_workspace_bytes", "deqsci_power_workspace_bytes",
                 "deqsci_broyden_workspace_bytes", "deqsci_broyden_chunk", "deqsci_epsilon2_workspace_bytes", "deqsci_epsilon2_chunk",
                 "deqsci_wgrad_workspace_bytes", "deqsci_wgrad_bn_workspace_bytes", "deqsci_realsn_workspace_bytes",
                 "deqsci_bn_train_workspace_bytes", "deqsci_mse_workspace_bytes", "deqsci_grad_norm_workspace_bytes")


class DeqsciHipError(RuntimeError):
    pass


def lib_path():
    return _LIB_PATH


def load():
    """Load libdeqsci_hip.so (after torch, so it binds to the HIP runtime torch already loaded)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise DeqsciHipError(
            f"{_LIB_PATH} is missing: build it with `make` (or __graft_entry__.build()). "
            "deqsci_amd has no CPU / eager fallback for its HIP kernels.")
    lib = ctypes.CDLL(_LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    for name, argtypes in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = _int
    lib.deqsci_version.restype = ctypes.c_char_p
    lib.deqsci_error_string.restype = ctypes.c_char_p
    lib.deqsci_error_string.argtypes = [_int]
    lib.deqsci_anderson_chunks.restype = _i64
    lib.deqsci_anderson_chunks.argtypes = [_i64, _i64]
    lib.deqsci_partials_bytes.restype = ctypes.c_size_t
    lib.deqsci_partials_bytes.argtypes = [_i64, _i64]
    lib.deqsci_gram_bytes.restype = ctypes.c_size_t
    lib.deqsci_gram_bytes.argtypes = [_i64]
    lib.deqsci_gram_ref_bytes.restype = ctypes.c_size_t
    lib.deqsci_gram_ref_bytes.argtypes = [_i64, _i64]
    lib.deqsci_ssim_workspace_bytes.restype = _i64
    lib.deqsci_ssim_workspace_bytes.argtypes = [_i64, _i64, _i64, _i64, _int]
    lib.deqsci_sqerr_workspace_bytes.restype = ctypes.c_size_t
    lib.deqsci_sqerr_workspace_bytes.argtypes = [_i64, _i64]
    lib.deqsci_power_workspace_bytes.restype = ctypes.c_size_t
    lib.deqsci_power_workspace_bytes.argtypes = [_i64, _i64]
    lib.deqsci_broyden_workspace_bytes.restype = ctypes.c_size_t
    lib.deqsci_broyden_workspace_bytes.argtypes = [_i64, _i64, _int]
    lib.deqsci_broyden_chunk.restype = _i64
    lib.deqsci_broyden_chunk.argtypes = []
    lib.deqsci_epsilon2_workspace_bytes.restype = ctypes.c_size_t
    lib.deqsci_epsilon2_workspace_bytes.argtypes = [_i64, _i64]
    lib.deqsci_epsilon2_chunk.restype = _i64
    lib.deqsci_epsilon2_chunk.argtypes = []
    lib.deqsci_wgrad_workspace_bytes.restype = ctypes.c_size_t
    lib.deqsci_wgrad_workspace_bytes.argtypes = [_i64, _i64, _i64]
    lib.deqsci_wgrad_bn_workspace_bytes.restype = ctypes.c_size_t
    lib.deqsci_wgrad_bn_workspace_bytes.argtypes = [_i64, _i64, _i64]
    lib.deqsci_realsn_workspace_bytes.restype = ctypes.c_size_t
    lib.deqsci_realsn_workspace_bytes.argtypes = [_i64, _i64, _i64, _i64]
    lib.deqsci_bn_train_workspace_bytes.restype = ctypes.c_size_t
    lib.deqsci_bn_train_workspace_bytes.argtypes = [_i64]
    lib.deqsci_mse_workspace_bytes.restype = ctypes.c_size_t
    lib.deqsci_mse_workspace_bytes.argtypes = [_i64]
    lib.deqsci_grad_norm_workspace_bytes.restype = ctypes.c_size_t
    lib.deqsci_grad_norm_workspace_bytes.argtypes = [_ptr, _i64]
    lib.deqsci_gaptv_workspace_bytes.restype = _i64
    lib.deqsci_gaptv_workspace_bytes.argtypes = [_i64, _i64, _i64, _i64]
    lib.deqsci_tv_chambolle_workspace_bytes.restype = _i64
    lib.deqsci_tv_chambolle_workspace_bytes.argtypes = [_i64, _i64, _i64]
    _lib = lib
    return lib


def _check(code, what):
    if code != 0:
        msg = load().deqsci_error_string(code).decode()
        raise DeqsciHipError(f"{what} failed with code {code}: {msg}")


def _p(t, name="tensor", allow_none=False):
    if t is None:
        if allow_none:
            return None
        raise DeqsciHipError(f"{name} is None")
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise DeqsciHipError(f"{name} must be a torch tensor on a HIP device (got "
                             f"{getattr(t, 'device', type(t))}); deqsci_amd has no CPU path")
    if t.dtype != torch.float32:
        raise DeqsciHipError(f"{name} must be float32, got {t.dtype}")
    if not t.is_contiguous():
        raise DeqsciHipError(f"{name} must be contiguous")
    return t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


class _NullCtx:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


_NULL = _NullCtx()


def _dev(t):
    """Device guard only when the tensor is not on the current device (the common case is free)."""
    if not t.is_cuda or t.device.index == torch.cuda.current_device():
        return _NULL
    return torch.cuda.device(t.device)


def f32c(t):
    """fp32 contiguous view/copy (the reference's tensors are fp32 throughout)."""
    if t.dtype != torch.float32:
        t = t.float()
    return t if t.is_contiguous() else t.contiguous()


def _dims(layout, shape):
    if layout == LAYOUT_HWB:
        bsz, H, W, B = shape
    else:
        bsz, B, H, W = shape
    return bsz, H, W, B


def _shape(layout, bsz, H, W, B):
    return (bsz, H, W, B) if layout == LAYOUT_HWB else (bsz, B, H, W)


def _phi_shared(phi, bsz):
    if phi.dim() == 3:
        return 1
    if phi.shape[0] == 1 and bsz > 1:
        return 1
    if phi.shape[0] != bsz:
        raise DeqsciHipError(f"Phi batch {phi.shape[0]} does not match batch {bsz}")
    return 0


# ----------------------------------------------------------------------------- operators
def sci_forward(x, phi, layout=LAYOUT_HWB, out=None):
    bsz, H, W, B = _dims(layout, x.shape)
    if tuple(phi.shape[-3:]) != tuple(x.shape[-3:]):
        raise DeqsciHipError(f"x {tuple(x.shape)} and Phi {tuple(phi.shape)} do not match")
    y = out if out is not None else torch.empty((bsz, H, W), device=x.device, dtype=torch.float32)
    with _dev(x):
        _check(load().deqsci_sci_forward_f32(_p(x, "x"), _p(phi, "Phi"), _p(y, "y"), bsz, H, W, B, layout,
                                             _phi_shared(phi, bsz), _stream()), "sci_forward")
    return y


def sci_adjoint(y, phi, layout=LAYOUT_HWB, out=None):
    bsz = y.shape[0]
    _, H, W, B = _dims(layout, (1,) + tuple(phi.shape[-3:]))
    if tuple(y.shape) != (bsz, H, W):
        raise DeqsciHipError(f"y {tuple(y.shape)} and Phi {tuple(phi.shape)} do not match")
    x = out if out is not None else torch.empty(_shape(layout, bsz, H, W, B), device=y.device, dtype=torch.float32)
    with _dev(y):
        _check(load().deqsci_sci_adjoint_f32(_p(y, "y"), _p(phi, "Phi"), _p(x, "x"), bsz, H, W, B, layout,
                                             _phi_shared(phi, bsz), _stream()), "sci_adjoint")
    return x


def phi_sum(phi, layout=LAYOUT_HWB):
    p4 = phi if phi.dim() == 4 else phi.unsqueeze(0)
    nb, H, W, B = _dims(layout, p4.shape)
    out = torch.empty((nb, H, W), device=phi.device, dtype=torch.float32)
    with _dev(phi):
        _check(load().deqsci_phi_sum_f32(_p(p4, "Phi"), _p(out), nb, H, W, B, layout, _stream()), "phi_sum")
    return out if phi.dim() == 4 else out[0]


def gap_update(z, phi, y, phisum, layout_in=LAYOUT_HWB, layout_out=None, out=None):
    layout_out = layout_in if layout_out is None else layout_out
    bsz, H, W, B = _dims(layout_in, z.shape)
    if tuple(phi.shape[-3:]) != tuple(z.shape[-3:]) or tuple(y.shape) != (bsz, H, W):
        raise DeqsciHipError(f"gap_update shapes z {tuple(z.shape)} Phi {tuple(phi.shape)} y {tuple(y.shape)}")
    shared = _phi_shared(phi, bsz)
    if phisum.numel() != (1 if shared else bsz) * H * W:
        raise DeqsciHipError(f"Phi_sum {tuple(phisum.shape)} does not match Phi {tuple(phi.shape)} (shared={shared})")
    z1 = out if out is not None else torch.empty(_shape(layout_out, bsz, H, W, B), device=z.device, dtype=torch.float32)
    with _dev(z):
        _check(load().deqsci_gap_update_f32(_p(z, "z"), _p(phi, "Phi"), _p(y, "y"), _p(phisum, "Phi_sum"), _p(z1, "z1"),
                                            bsz, H, W, B, layout_in, layout_out, _phi_shared(phi, bsz), _stream()),
               "gap_update")
    return z1


def gap_update_grad(z, phi, g, y, phisum, need=(True, True, False, False), out=None):
    """G1, the backward of gap_update in one launch (HWB): (gphi, gs, gz, gy) for g = the gradient of z1, None where `need` is false.
    gphi has Phi's shape and gs Phi_sum's; a shared mask's hold the sum over the batch.  out: four tensors or None, used where given."""
    bsz, H, W, B = z.shape
    if tuple(phi.shape[-3:]) != (H, W, B) or tuple(g.shape) != (bsz, H, W, B) or tuple(y.shape) != (bsz, H, W):
        raise DeqsciHipError(f"gap_update_grad shapes z {tuple(z.shape)} Phi {tuple(phi.shape)} g {tuple(g.shape)} y {tuple(y.shape)}")
    shared = _phi_shared(phi, bsz)
    nm = 1 if shared else bsz
    if phisum.numel() != nm * H * W:
        raise DeqsciHipError(f"Phi_sum {tuple(phisum.shape)} does not match Phi {tuple(phi.shape)} (shared={shared})")
    if not any(need):
        raise DeqsciHipError("gap_update_grad: no output asked for")
    shapes = (tuple(phi.shape), tuple(phisum.shape), (bsz, H, W, B), (bsz, H, W))
    out = out or (None,) * 4
    outs = [(o if o is not None else torch.empty(s, device=z.device, dtype=torch.float32)) if want else None
            for want, s, o in zip(need, shapes, out)]
    with _dev(z):
        _check(load().deqsci_gap_update_grad_f32(_p(z, "z"), _p(phi, "Phi"), _p(g, "g"), _p(y, "y"), _p(phisum, "Phi_sum"),
                                                 *[_p(o, allow_none=True) for o in outs], bsz, H, W, B, LAYOUT_HWB, shared, _stream()),
               "gap_update_grad")
    return tuple(outs)


def sci_mask_grad(a, v, phi_shape, out=None):
    """G2 (HWB): gphi_b = a v_b in the shape of the mask - (bsz,H,W,B) per measurement; (1,H,W,B) or (H,W,B): summed over the batch."""
    bsz, H, W, B = v.shape
    phi_shape = tuple(phi_shape)
    if tuple(a.shape) != (bsz, H, W) or phi_shape[-3:] != (H, W, B):
        raise DeqsciHipError(f"sci_mask_grad shapes a {tuple(a.shape)} v {tuple(v.shape)} Phi {phi_shape}")
    shared = 1 if len(phi_shape) == 3 or (phi_shape[0] == 1 and bsz > 1) else 0
    if not shared and phi_shape[0] != bsz:
        raise DeqsciHipError(f"Phi batch {phi_shape[0]} does not match batch {bsz}")
    gphi = out if out is not None else torch.empty(phi_shape, device=v.device, dtype=torch.float32)
    with _dev(v):
        _check(load().deqsci_sci_mask_grad_f32(_p(a, "a"), _p(v, "v"), _p(gphi, "gphi"), bsz, H, W, B, LAYOUT_HWB, shared, _stream()),
               "sci_mask_grad")
    return gphi


def phi_sum_grad(phi, gs, out=None):
    """G3 (HWB): the backward of phi_sum - gs spread over the frames, 0 where the sum of the mask is 0 (phi_sum wrote 1 there)."""
    p4 = phi if phi.dim() == 4 else phi.unsqueeze(0)
    nb, H, W, B = p4.shape
    if gs.numel() != nb * H * W:
        raise DeqsciHipError(f"phi_sum_grad shapes Phi {tuple(phi.shape)} gs {tuple(gs.shape)}")
    gphi = out if out is not None else torch.empty(tuple(phi.shape), device=phi.device, dtype=torch.float32)
    with _dev(phi):
        _check(load().deqsci_phi_sum_grad_f32(_p(p4, "Phi"), _p(gs, "gs"), _p(gphi, "gphi"), nb, H, W, B, LAYOUT_HWB, _stream()), "phi_sum_grad")
    return gphi


def transpose(t, to_layout, out=None):
    """(bsz,H,W,B) -> (bsz,B,H,W) when to_layout == LAYOUT_BHW, and back."""
    from_layout = LAYOUT_HWB if to_layout == LAYOUT_BHW else LAYOUT_BHW
    bsz, H, W, B = _dims(from_layout, t.shape)
    o = out if out is not None else torch.empty(_shape(to_layout, bsz, H, W, B), device=t.device, dtype=torch.float32)
    with _dev(t):
        _check(load().deqsci_transpose_f32(_p(t, "in"), _p(o, "out"), bsz, H, W, B, to_layout, _stream()), "transpose")
    return o


def residual_out(z1, noise, layout_out=LAYOUT_HWB, out=None):
    """out = z1 - noise; z1, noise planar (bsz,B,H,W); out in layout_out."""
    bsz, B, H, W = z1.shape
    o = out if out is not None else torch.empty(_shape(layout_out, bsz, H, W, B), device=z1.device, dtype=torch.float32)
    with _dev(z1):
        code = load().deqsci_residual_out_f32(_p(z1, "z1"), _p(noise, "noise"), _p(o, "out"), bsz, H, W, B, layout_out, _stream())
    if code == -4 and layout_out == LAYOUT_HWB:       # odd B / H*W: planar subtract, then the generic LDS transpose
        tmp = residual_out(z1, noise, LAYOUT_BHW)
        return transpose(tmp, LAYOUT_HWB, out=o)
    _check(code, "residual_out")
    return o


# ----------------------------------------------------------------------------- Anderson workspace + steps
class AndersonWorkspace:
    """Caller-owned buffers for K4-K7 (the library never allocates)."""

    def __init__(self, bsz, N, m, device, res_rows=1):
        if m > MAX_M:
            raise DeqsciHipError(f"Anderson history m={m} exceeds DEQSCI_MAX_M={MAX_M}")
        lib = load()
        self.bsz, self.N, self.m = bsz, N, m
        self.F = torch.zeros((bsz, m, N), device=device, dtype=torch.float32)
        self.G = torch.zeros((bsz, m, N), device=device, dtype=torch.float32)
        self.nchunks = lib.deqsci_anderson_chunks(bsz, N)
        self.partials = torch.empty(lib.deqsci_partials_bytes(bsz, N) // 4, device=device, dtype=torch.float32)
        self.gram = torch.zeros(lib.deqsci_gram_bytes(bsz) // 8, device=device, dtype=torch.float64)
        self.alpha = torch.zeros((bsz, MAX_M), device=device, dtype=torch.float32)
        self.res = torch.zeros((res_rows, 1 + bsz), device=device, dtype=torch.float32)
        self.gram32 = None                # (anderson_arith = "reference": the persistent fp32 Gram of deqsci_anderson_solve_ref_f32, see gram32_state)
        self.ref_fusable = bool(lib.deqsci_gram_ref_fusable(bsz, N))      # K4 can leave the records of the reference Gram's first pass itself
        self._rounded = None              # (slot, n_filled) of a residual_store(ref=True) whose records await anderson_solve(ref=True)

    def ref_state(self):
        """The caller-owned state of deqsci_anderson_solve_ref_f32 (allocated and zeroed on first use): per sample the persistent fp32 Gram
        (MAX_M x MAX_M), the 16 chain sums per entry of the last call, and the block records of the two-pass form."""
        if self.gram32 is None:
            self.gram32 = torch.zeros(load().deqsci_gram_ref_bytes(self.bsz, self.N) // 4, device=self.F.device, dtype=torch.float32)
        return self.gram32

    def gram32_state(self):
        """(bsz, MAX_M, MAX_M) view of the persistent fp32 Gram in ref_state()."""
        st = self.ref_state().view(self.bsz, -1)
        return st[:, :MAX_M * MAX_M].view(self.bsz, MAX_M, MAX_M)

    def chain_sums(self):
        """(bsz, MAX_M, 16) view of the chain sums of the last deqsci_gram_row_chain16_f32 / deqsci_anderson_solve_ref_f32 call."""
        st = self.ref_state().view(self.bsz, -1)
        return st[:, MAX_M * MAX_M:MAX_M * MAX_M + 16 * MAX_M].view(self.bsz, MAX_M, 16)

    def chains_walked(self):
        """(bsz, MAX_M, 16) int32 view (diagnostic): the blocks each chain was walked through term by term in the last two-pass call (-1: serial form)."""
        st = self.ref_state().view(self.bsz, -1)
        return st[:, MAX_M * MAX_M + 16 * MAX_M:MAX_M * MAX_M + 32 * MAX_M].view(torch.int32).view(self.bsz, MAX_M, 16)


def residual_store(ws, z1, noise, x_cur, slot, n_filled, x_next=None, ref=False):
    """ref: the caller will form alpha with anderson_solve(ref=True) next - where the shape allows (ws.ref_fusable) K4's blocks then also leave
    the records of the reference Gram's first pass (deqsci_residual_store_ref_f32: the history rows are in their registers anyway), and
    that anderson_solve skips the pass.  Same F / G / x_next / partials either way."""
    ws._rounded = None
    if ref and ws.ref_fusable:
        with _dev(z1):
            _check(load().deqsci_residual_store_ref_f32(_p(z1, "z1"), _p(noise, "noise", True), _p(x_cur, "x_cur"), _p(ws.F), _p(ws.G),
                                                        _p(x_next, "x_next", True), _p(ws.partials), _p(ws.ref_state()), ws.bsz, ws.N, ws.m, slot,
                                                        n_filled, _stream()), "residual_store_ref")
        ws._rounded = (slot, n_filled)
        return
    with _dev(z1):
        _check(load().deqsci_residual_store_f32(_p(z1, "z1"), _p(noise, "noise", True), _p(x_cur, "x_cur"), _p(ws.F), _p(ws.G),
                                                _p(x_next, "x_next", True), _p(ws.partials), ws.bsz, ws.N, ws.m, slot,
                                                n_filled, _stream()), "residual_store")


def anderson_solve(ws, slot, n_filled, n, lam, eps, res_row=0, gram32=None, ref=False):
    """gram32: (bsz, n, n) fp32 - alpha from THAT Gram block with an fp32 LU (the reference's arithmetic, :177-180) instead of the float64 sums.
    ref: the same arithmetic without a GEMM library - the new Gram row summed by the build's own kernel in the order of the reference's torch.bmm
    (sixteen interleaved FMA chains per entry, csrc/anderson.hip gram_row_chain16_kernel) from the history residual_store just wrote."""
    if ref and ws._rounded == (slot, n_filled):
        ws._rounded = None
        with _dev(ws.F):
            _check(load().deqsci_anderson_apply_solve_ref_f32(_p(ws.G), _p(ws.partials), _p(ws.ref_state()), ws.gram.data_ptr(), _p(ws.alpha),
                                                              _p(ws.res[res_row]), ws.bsz, ws.N, ws.m, slot, n_filled, n, float(lam), float(eps), _stream()),
                   "anderson_apply_solve_ref")
        return
    ws._rounded = None
    if ref:
        with _dev(ws.F):
            _check(load().deqsci_anderson_solve_ref_f32(_p(ws.G), _p(ws.partials), _p(ws.ref_state()), ws.gram.data_ptr(), _p(ws.alpha),
                                                        _p(ws.res[res_row]), ws.bsz, ws.N, ws.m, slot, n_filled, n, float(lam), float(eps), _stream()),
                   "anderson_solve_ref")
        return
    if gram32 is not None and (tuple(gram32.shape) != (ws.bsz, n, n) or gram32.dtype != torch.float32 or not gram32.is_contiguous() or not gram32.is_cuda):
        raise DeqsciHipError(f"anderson_solve: gram32 must be a contiguous fp32 GPU tensor of shape {(ws.bsz, n, n)}")
    with _dev(ws.F):
        _check(load().deqsci_anderson_solve_gram_f32(_p(ws.partials), ws.gram.data_ptr(), _p(ws.alpha), _p(ws.res[res_row]),
                                                     ws.bsz, ws.N, ws.m, slot, n_filled, n, float(lam), float(eps),
                                                     None if gram32 is None else gram32.data_ptr(), _stream()), "anderson_solve")


def gram_row_chain16(ws, slot, n_filled, serial=False):
    """The 16 chain sums of every entry of the new Gram row (ws.chain_sums()) from the history and block sums residual_store just wrote:
    serial=True as the chains are written, False in the two-pass form (the same bits; tests hold them equal)."""
    with _dev(ws.F):
        _check(load().deqsci_gram_row_chain16_f32(_p(ws.G), _p(ws.partials), _p(ws.ref_state()), ws.bsz, ws.N, ws.m, slot, n_filled, int(bool(serial)),
                                                  _stream()), "gram_row_chain16")
    return ws.chain_sums()


def anderson_mix(ws, x_out, beta, n):
    with _dev(ws.F):
        _check(load().deqsci_anderson_mix_f32(_p(ws.F), _p(ws.G), _p(ws.alpha), _p(x_out, "x_out"), float(beta), n,
                                              ws.bsz, ws.N, ws.m, _stream()), "anderson_mix")


def anderson_mix_gap(ws, beta, n, phi, y, phisum, x_out, z1, layout):
    bsz, H, W, B = _dims(layout, z1.shape)
    with _dev(ws.F):
        _check(load().deqsci_anderson_mix_gap_f32(_p(ws.F), _p(ws.G), _p(ws.alpha), float(beta), n, ws.m, _p(phi, "Phi"),
                                                  _p(y, "y"), _p(phisum, "Phi_sum"), _p(x_out, "x_out"), _p(z1, "z1"),
                                                  bsz, H, W, B, layout, _phi_shared(phi, bsz), _stream()), "anderson_mix_gap")


def bias_relu_(h, bias, relu=True):
    """In-place h = max(h + bias[c], 0) for a 4-D activation, NCHW-contiguous or channels_last."""
    n, c, hh, ww = h.shape
    if h.is_contiguous():
        cl = 0
    elif h.is_contiguous(memory_format=torch.channels_last):
        cl = 1
    else:
        raise DeqsciHipError("bias_relu_: activation must be contiguous (NCHW or channels_last)")
    if h.dtype != torch.float32 or not h.is_cuda:
        raise DeqsciHipError("bias_relu_: fp32 GPU tensor required")
    with _dev(h):
        _check(load().deqsci_bias_relu_f32(h.data_ptr(), _p(bias, "bias"), n, c, hh * ww, cl, 1 if relu else 0, _stream()),
               "bias_relu")
    return h


def pack_tail_weights(w):
    """(4,64,3,3) conv weight -> [half(2)][tap(9)][cin(32)][cout(4)] for deqsci_ffdnet_tail_f32."""
    if tuple(w.shape) != (4, 64, 3, 3):
        raise DeqsciHipError(f"ffdnet tail expects a (4,64,3,3) weight, got {tuple(w.shape)}")
    return w.detach().float().permute(2, 3, 1, 0).reshape(9, 2, 32, 4).permute(1, 0, 2, 3).contiguous()


def ffdnet_tail(h, w_packed, out=None, in_bias=None):
    """h (n,64,H,W) channels_last -> planar noise (n,1,2H,2W) = pixel_shuffle(conv3x3(h', w, pad=1), 2) with
    h' = h, or relu(h + in_bias[c]) when in_bias is given (previous layer's epilogue fused into the read).  (An Sp16 activation goes to
    tail_split16.)"""
    n, c, H, W = h.shape
    if c != 64 or not h.is_contiguous(memory_format=torch.channels_last) or h.dtype != torch.float32 or not h.is_cuda:
        raise DeqsciHipError("ffdnet_tail: fp32 channels_last GPU activation with 64 channels required")
    o = out if out is not None else torch.empty((n, 1, 2 * H, 2 * W), device=h.device, dtype=torch.float32)
    with _dev(h):
        _check(load().deqsci_ffdnet_tail_f32(h.data_ptr(), _p(w_packed, "w_packed"), _p(in_bias, "in_bias", True), _p(o, "out"),
                                             n, H, W, _stream()), "ffdnet_tail")
    return o


def pack_c64_to_1_weights(w):
    """(1,64,3,3) conv weight -> [half(2)][tap(9)][cin(32)] for deqsci_conv3x3_c64_to_1_f32."""
    if tuple(w.shape) != (1, 64, 3, 3):
        raise DeqsciHipError(f"expected a (1,64,3,3) weight, got {tuple(w.shape)}")
    return w.detach().float().permute(2, 3, 1, 0).reshape(9, 2, 32).permute(1, 0, 2).contiguous()


def conv3x3_c64_to_1(h, w_packed, out=None, in_bias=None):
    """h (n,64,H,W) channels_last -> planar (n,1,H,W) = conv3x3(h', w, pad=1), h' = h or relu(h + in_bias[c]).  (An Sp16 activation
    goes to tail_split16.)"""
    n, c, H, W = h.shape
    if c != 64 or not h.is_contiguous(memory_format=torch.channels_last) or h.dtype != torch.float32 or not h.is_cuda:
        raise DeqsciHipError("conv3x3_c64_to_1: fp32 channels_last GPU activation with 64 channels required")
    o = out if out is not None else torch.empty((n, 1, H, W), device=h.device, dtype=torch.float32)
    with _dev(h):
        _check(load().deqsci_conv3x3_c64_to_1_f32(h.data_ptr(), _p(w_packed, "w_packed"), _p(in_bias, "in_bias", True), _p(o, "out"),
                                                  n, H, W, _stream()), "conv3x3_c64_to_1")
    return o


def pack_c1_to_64_weights(w):
    """(64,1,3,3) conv weight -> [tap(9)][cout//4(16)][cout%4(4)] for deqsci_conv3x3_c1_to_64_f32."""
    if tuple(w.shape) != (64, 1, 3, 3):
        raise DeqsciHipError(f"expected a (64,1,3,3) weight, got {tuple(w.shape)}")
    return w.detach().float().reshape(16, 4, 9).permute(2, 0, 1).contiguous()


def conv3x3_c1_to_64(x, w_packed, relu=True, out=None, sp16=False, out_rng=None, out_exp=None, track=None, p32=False):
    """x (n,1,H,W) planar -> [relu](conv3x3(x, w, pad=1)) as a channels_last (n,64,H,W) activation, or as an Sp16 (sp16=True) / a P32
    (p32=True: in front of conv3x3_c64_wino16 layers) with the range (out_rng, out_exp); track: a range slot that receives max |output|
    (the measurement of the first f-call)."""
    n, c, H, W = x.shape
    if c != 1:
        raise DeqsciHipError(f"conv3x3_c1_to_64: (n,1,H,W) image required, got {tuple(x.shape)}")
    if p32:
        o = out if out is not None else P32.empty(n, H, W, x.device)
        if not isinstance(o, P32) or (o.n, o.H, o.W) != (n, H, W):
            raise DeqsciHipError("conv3x3_c1_to_64: out must be a P32 of the output's shape")
        o.rng, o.exp = out_rng, SP16_DEFAULT_EXP if out_exp is None else int(out_exp)
        with _dev(x):
            _check(load().deqsci_conv3x3_c1_to_64_p32(_p(x, "x"), _p(w_packed, "w_packed"), o.t.data_ptr(), n, H, W, 1 if relu else 0,
                                                      _rng(o.rng, n), o.exp, _rng(track, n), _stream()), "conv3x3_c1_to_64_p32")
        return o
    if sp16:
        o = out if out is not None else Sp16.empty(n, H, W, x.device)
        o.rng, o.exp = out_rng, SP16_DEFAULT_EXP if out_exp is None else int(out_exp)
        with _dev(x):
            _check(load().deqsci_conv3x3_c1_to_64_sp16(_p(x, "x"), _p(w_packed, "w_packed"), o.t.data_ptr(), n, H, W, 1 if relu else 0,
                                                       _rng(o.rng, n), o.exp, _rng(track, n), _stream()), "conv3x3_c1_to_64_sp16")
        return o
    o = out if out is not None else torch.empty((n, 64, H, W), device=x.device, dtype=torch.float32, memory_format=torch.channels_last)
    with _dev(x):
        _check(load().deqsci_conv3x3_c1_to_64_f32(_p(x, "x"), _p(w_packed, "w_packed"), o.data_ptr(), n, H, W, 1 if relu else 0,
                                                  _stream()), "conv3x3_c1_to_64")
    return o


def relu_mask_pack(a, out=None):
    """fp32 channels_last (n,64,H,W) activation -> (n,H,W) int64 words, bit c = (a[:, c] > 0) (csrc/vjp.hip: the implicit backward's
    ReLU masks; +-0.0 and NaN give 0)."""
    n, c, H, W = a.shape
    if c != 64 or not a.is_contiguous(memory_format=torch.channels_last) or a.dtype != torch.float32 or not a.is_cuda:
        raise DeqsciHipError("relu_mask_pack: fp32 channels_last GPU activation with 64 channels required")
    o = out if out is not None else torch.empty((n, H, W), device=a.device, dtype=torch.int64)
    if tuple(o.shape) != (n, H, W) or o.dtype != torch.int64 or not o.is_contiguous() or o.device != a.device:
        raise DeqsciHipError("relu_mask_pack: out must be a contiguous int64 (n,H,W) tensor on the activation's device")
    with _dev(a):
        _check(load().deqsci_relu_mask_pack_f32(a.data_ptr(), o.data_ptr(), n * H * W, _stream()), "relu_mask_pack")
    return o


def wgrad_workspace(n, H, W, device):
    """The scratch buffer of wgrad_c64_c64 / wgrad_c1_c64 for (n,H,W) images (deqsci_wgrad_workspace_bytes; serves both, uninitialised)."""
    nbytes = load().deqsci_wgrad_workspace_bytes(n, H, W)
    if nbytes == 0:
        raise DeqsciHipError(f"wgrad_workspace: sizes {(n, H, W)} are not served")
    return torch.empty(nbytes // 8, device=device, dtype=torch.float64)


def _wgrad_ws(workspace, n, H, W, ref, what):
    ws = workspace if workspace is not None else wgrad_workspace(n, H, W, ref.device)
    if (not isinstance(ws, torch.Tensor) or not ws.is_cuda or ws.device != ref.device or not ws.is_contiguous()
            or ws.numel() * ws.element_size() < load().deqsci_wgrad_workspace_bytes(n, H, W)):
        raise DeqsciHipError(f"{what}: workspace must be a contiguous tensor of wgrad_workspace{(n, H, W)}'s size on the inputs' device")
    return ws


def _act64(a, what, name):
    if (not isinstance(a, torch.Tensor) or a.dim() != 4 or a.shape[1] != 64 or not a.is_cuda or a.dtype != torch.float32
            or not a.is_contiguous(memory_format=torch.channels_last)):
        raise DeqsciHipError(f"{what}: {name} must be an fp32 channels_last (n,64,H,W) GPU activation")
    return a


def wgrad_c64_c64(x, g, workspace=None):
    """The weight gradient of a 64 -> 64 conv3x3 (pad 1): dw[co,ci,ky,kx] = sum g[:,co,h,w] x[:,ci,h+ky-1,w+kx-1], x the layer's input and
    g the gradient behind it, both fp32 channels_last (n,64,H,W) -> (64,64,3,3) (csrc/wgrad.hip W0; deterministic)."""
    _act64(x, "wgrad_c64_c64", "x"), _act64(g, "wgrad_c64_c64", "g")
    if x.shape != g.shape or x.device != g.device:
        raise DeqsciHipError(f"wgrad_c64_c64: x {tuple(x.shape)} and g {tuple(g.shape)} must have one shape and device")
    n, _, H, W = x.shape
    ws = _wgrad_ws(workspace, n, H, W, x, "wgrad_c64_c64")
    dw = torch.empty((64, 64, 3, 3), device=x.device, dtype=torch.float32)
    with _dev(x):
        _check(load().deqsci_wgrad3x3_c64_c64_f32(x.data_ptr(), g.data_ptr(), dw.data_ptr(), n, H, W, ws.data_ptr(), _stream()), "wgrad_c64_c64")
    return dw


def wgrad_c1_c64(s, t, flip, workspace=None):
    """The weight gradient of an edge layer from the planar (n,1,H,W) image s and the channels_last (n,64,H,W) activation t (csrc/wgrad.hip W1):
    flip = 0 -> (64,1,3,3), dw[c,0,ky,kx] = sum t[:,c,h,w] s[:,0,h+ky-1,w+kx-1] (first layer: s its input, t the gradient behind it);
    flip = 1 -> (1,64,3,3), dw[0,c,ky,kx] = sum s[:,0,h,w] t[:,c,h+ky-1,w+kx-1] (last layer: s the gradient behind it, t its input)."""
    _act64(t, "wgrad_c1_c64", "t")
    n, _, H, W = t.shape
    if tuple(s.shape) != (n, 1, H, W) or s.device != t.device:
        raise DeqsciHipError(f"wgrad_c1_c64: s must be the (n,1,H,W) = {(n, 1, H, W)} image on t's device, got {tuple(s.shape)}")
    if flip not in (0, 1):
        raise DeqsciHipError(f"wgrad_c1_c64: flip must be 0 or 1, got {flip!r}")
    ws = _wgrad_ws(workspace, n, H, W, t, "wgrad_c1_c64")
    dw = torch.empty((1, 64, 3, 3) if flip else (64, 1, 3, 3), device=t.device, dtype=torch.float32)
    with _dev(t):
        _check(load().deqsci_wgrad3x3_c1_c64_f32(_p(s, "s"), t.data_ptr(), dw.data_ptr(), int(flip), n, H, W, ws.data_ptr(), _stream()), "wgrad_c1_c64")
    return dw


def wgrad_bn_workspace(n, H, W, device):
    """The scratch buffer of wgrad_c64_c64_bn / wgrad_shuffle for (n,64,H,W) activations (deqsci_wgrad_bn_workspace_bytes; serves both,
    uninitialised)."""
    nbytes = load().deqsci_wgrad_bn_workspace_bytes(n, H, W)
    if nbytes == 0:
        raise DeqsciHipError(f"wgrad_bn_workspace: sizes {(n, H, W)} are not served")
    return torch.empty(nbytes // 8, device=device, dtype=torch.float64)


def _wgrad_bn_ws(workspace, n, H, W, ref, what):
    ws = workspace if workspace is not None else wgrad_bn_workspace(n, H, W, ref.device)
    if (not isinstance(ws, torch.Tensor) or not ws.is_cuda or ws.device != ref.device or not ws.is_contiguous()
            or ws.numel() * ws.element_size() < load().deqsci_wgrad_bn_workspace_bytes(n, H, W)):
        raise DeqsciHipError(f"{what}: workspace must be a contiguous tensor of wgrad_bn_workspace{(n, H, W)}'s size on the inputs' device")
    return ws


def wgrad_c64_c64_bn(x, g, w, scale, workspace=None):
    """A 64 -> 64 conv3x3 behind a frozen BatchNorm, y = relu(scale[co] conv(x, w) + shift) (csrc/wgrad_bn.hip W0-BN; deterministic): with
    R = wgrad_c64_c64(x, g) -> (dw, dsum, ddot) = ((float)(scale[co] R) (64,64,3,3), sum_p g[p,co] (64,), sum_{ci,tap} w R (64,)), formed in
    float64 from R's entry sums and rounded once.  w (64,64,3,3) and scale (64,) fp32 contiguous on x's device."""
    _act64(x, "wgrad_c64_c64_bn", "x"), _act64(g, "wgrad_c64_c64_bn", "g")
    if x.shape != g.shape or x.device != g.device:
        raise DeqsciHipError(f"wgrad_c64_c64_bn: x {tuple(x.shape)} and g {tuple(g.shape)} must have one shape and device")
    if tuple(w.shape) != (64, 64, 3, 3) or tuple(scale.shape) != (64,) or w.device != x.device or scale.device != x.device:
        raise DeqsciHipError(f"wgrad_c64_c64_bn: w must be (64,64,3,3) and scale (64,) on x's device, got {tuple(w.shape)}, {tuple(scale.shape)}")
    n, _, H, W = x.shape
    ws = _wgrad_bn_ws(workspace, n, H, W, x, "wgrad_c64_c64_bn")
    dw = torch.empty((64, 64, 3, 3), device=x.device, dtype=torch.float32)
    dsum, ddot = torch.empty(64, device=x.device, dtype=torch.float32), torch.empty(64, device=x.device, dtype=torch.float32)
    with _dev(x):
        _check(load().deqsci_wgrad3x3_c64_c64_bn_f32(x.data_ptr(), g.data_ptr(), _p(w, "w"), _p(scale, "scale"), dw.data_ptr(), dsum.data_ptr(),
                                                     ddot.data_ptr(), n, H, W, ws.data_ptr(), _stream()), "wgrad_c64_c64_bn")
    return dw, dsum, ddot


def wgrad_shuffle(img, t, which, sigma=None, workspace=None):
    """The weight gradient of an FFDNet edge layer, read through the 2x2 pixel-unshuffle u of the planar (n,1,2H,2W) image img; t the
    channels_last (n,64,H,W) activation (csrc/wgrad_bn.hip W2):
    which = 0 -> (64,5,3,3): channels 1..4 sum t[:,c,p] u[:,q,p+d] (img the layer's input, t the masked gradient behind it), channel 0
                 sum sigma[img] t[:,c,p] over the taps inside the image - sigma (1,) or (n,) fp32 on the device;
    which = 1 -> (4,64,3,3): sum u[:,q,p] t[:,c,p+d] (img the gradient of the noise, t the last activation)."""
    _act64(t, "wgrad_shuffle", "t")
    n, _, H, W = t.shape
    if tuple(img.shape) != (n, 1, 2 * H, 2 * W) or img.device != t.device:
        raise DeqsciHipError(f"wgrad_shuffle: img must be the (n,1,2H,2W) = {(n, 1, 2 * H, 2 * W)} image on t's device, got {tuple(img.shape)}")
    if which not in (0, 1):
        raise DeqsciHipError(f"wgrad_shuffle: which must be 0 or 1, got {which!r}")
    sp, stride = None, 0
    if which == 0:
        if (not isinstance(sigma, torch.Tensor) or sigma.device != t.device or sigma.dtype != torch.float32 or sigma.dim() != 1
                or sigma.numel() not in (1, n) or (sigma.numel() > 1 and sigma.stride(0) not in (0, 1))):
            raise DeqsciHipError("wgrad_shuffle: which = 0 needs sigma, a fp32 GPU vector of 1 or n elements")
        sp, stride = sigma.data_ptr(), (0 if sigma.numel() == 1 else sigma.stride(0))
    ws = _wgrad_bn_ws(workspace, n, H, W, t, "wgrad_shuffle")
    dw = torch.empty((4, 64, 3, 3) if which else (64, 5, 3, 3), device=t.device, dtype=torch.float32)
    with _dev(t):
        _check(load().deqsci_wgrad3x3_shuffle_f32(_p(img, "img"), sp, stride, t.data_ptr(), dw.data_ptr(), int(which), n, 2 * H, 2 * W,
                                                  ws.data_ptr(), _stream()), "wgrad_shuffle")
    return dw


def _mask_ptr(mask, n, H, W, what):
    if (not isinstance(mask, torch.Tensor) or tuple(mask.shape) != (n, H, W) or mask.dtype != torch.int64 or not mask.is_cuda
            or not mask.is_contiguous()):
        raise DeqsciHipError(f"{what}: mask must be the contiguous int64 (n,H,W) = {(n, H, W)} GPU tensor of relu_mask_pack")
    return mask.data_ptr()


# ----------------------------------------------------------------------------- BatchNorm2d in train mode (csrc/bn_train.hip)
def bn_train_workspace(P, device):
    """The scratch buffer of bn_train_stats / bn_train_grad_stats for P pixels (deqsci_bn_train_workspace_bytes; uninitialised)."""
    nbytes = load().deqsci_bn_train_workspace_bytes(P)
    if nbytes == 0:
        raise DeqsciHipError(f"bn_train_workspace: {P} pixels are not served (torch: expected more than 1 value per channel when training)")
    return torch.empty(nbytes // 8, dtype=torch.float64, device=device)


def _bn_ws(workspace, P, ref, what):
    ws = workspace if workspace is not None else bn_train_workspace(P, ref.device)
    if (ws.device != ref.device or not ws.is_contiguous() or ws.data_ptr() % 8
            or ws.numel() * ws.element_size() < load().deqsci_bn_train_workspace_bytes(P)):
        raise DeqsciHipError(f"{what}: workspace must be a contiguous tensor of bn_train_workspace({P})'s size on the activation's device")
    return ws


def _bn_vec(t, dtype, numel, ref, what, name):
    if (not isinstance(t, torch.Tensor) or t.dtype != dtype or t.numel() != numel or not t.is_contiguous() or t.device != ref.device):
        raise DeqsciHipError(f"{what}: {name} must be a contiguous {dtype} tensor of {numel} elements on the activation's device")
    return t.data_ptr()


def bn_train_stats(c, running_mean=None, running_var=None, num_batches_tracked=None, momentum=0.1, record=None, workspace=None):
    """T1: the batch mean and BIASED variance per channel of the fp32 channels_last (n,64,H,W) activation c, in float64 -> record (128,)
    float64 = mean, var.  running_mean, running_var (fp32 (64,)) and num_batches_tracked (int64 scalar), all three or none, are updated IN
    PLACE as torch's train-mode BatchNorm2d does.  4 launches, no host synchronisation."""
    _act64(c, "bn_train_stats", "c")
    n, _, H, W = c.shape
    P = n * H * W
    bufs = (running_mean, running_var, num_batches_tracked)
    if any(b is None for b in bufs) and not all(b is None for b in bufs):
        raise DeqsciHipError("bn_train_stats: running_mean, running_var and num_batches_tracked go together: all three or none")
    rec = torch.empty(128, dtype=torch.float64, device=c.device) if record is None else record
    rp = _bn_vec(rec, torch.float64, 128, c, "bn_train_stats", "record")
    if bufs[0] is None:
        rm = rv = nbt = None
    else:
        rm = _bn_vec(running_mean, torch.float32, 64, c, "bn_train_stats", "running_mean")
        rv = _bn_vec(running_var, torch.float32, 64, c, "bn_train_stats", "running_var")
        nbt = _bn_vec(num_batches_tracked, torch.int64, 1, c, "bn_train_stats", "num_batches_tracked")
    ws = _bn_ws(workspace, P, c, "bn_train_stats")
    with _dev(c):
        _check(load().deqsci_bn_train_stats_f32(c.data_ptr(), rp, rm, rv, nbt, float(momentum), P, ws.data_ptr(), _stream()), "bn_train_stats")
    return rec


def bn_train_apply(c, record, gamma, beta, eps, relu=True, out=None, mask=None, want_mask=False):
    """T2: y = relu?(gamma (c - mean) / sqrt(var + eps) + beta) from T1's record (the order of operations: include/deqsci_hip.h) as a
    channels_last (n,64,H,W) activation; out may be c.  want_mask / mask: relu_mask_pack's (n,H,W) int64 words of y, written in the same
    pass.  -> y, or (y, mask).  1 launch."""
    _act64(c, "bn_train_apply", "c")
    n, _, H, W = c.shape
    o = torch.empty_like(c, memory_format=torch.channels_last) if out is None else out
    if o is not c:
        _act64(o, "bn_train_apply", "out")
        if o.shape != c.shape or o.device != c.device:
            raise DeqsciHipError(f"bn_train_apply: out {tuple(o.shape)} must have c's shape {tuple(c.shape)} and device")
    if mask is None and want_mask:
        mask = torch.empty((n, H, W), dtype=torch.int64, device=c.device)
    mp = None if mask is None else _mask_ptr(mask, n, H, W, "bn_train_apply")
    rp = _bn_vec(record, torch.float64, 128, c, "bn_train_apply", "record")
    gp, bp = _bn_vec(gamma, torch.float32, 64, c, "bn_train_apply", "gamma"), _bn_vec(beta, torch.float32, 64, c, "bn_train_apply", "beta")
    with _dev(c):
        _check(load().deqsci_bn_train_apply_f32(c.data_ptr(), rp, gp, bp, float(eps), o.data_ptr(), mp, 1 if relu else 0, n * H * W, _stream()),
               "bn_train_apply")
    return o if mask is None else (o, mask)


def bn_train_grad_stats(gy, c, record, eps, workspace=None, out=None):
    """T3: from the (already ReLU-masked) gradient gy behind the layer and the stored convolution output c -> (dgamma, dbeta, grad_record):
    dbeta = sum gy, dgamma = sum gy (c - mean) / sqrt(var + eps) in float64 (grad_record (128,) = dbeta, dgamma), rounded once to the two
    fp32 (64,) outputs.  out: the three tensors to write instead of new ones.  2 launches."""
    _act64(gy, "bn_train_grad_stats", "gy"), _act64(c, "bn_train_grad_stats", "c")
    if gy.shape != c.shape or gy.device != c.device:
        raise DeqsciHipError(f"bn_train_grad_stats: gy {tuple(gy.shape)} and c {tuple(c.shape)} must have one shape and device")
    n, _, H, W = c.shape
    rp = _bn_vec(record, torch.float64, 128, c, "bn_train_grad_stats", "record")
    if out is None:
        grec = torch.empty(128, dtype=torch.float64, device=c.device)
        dgamma, dbeta = torch.empty(64, dtype=torch.float32, device=c.device), torch.empty(64, dtype=torch.float32, device=c.device)
    else:
        dgamma, dbeta, grec = out
        _bn_vec(dgamma, torch.float32, 64, c, "bn_train_grad_stats", "out[0] (dgamma)"), _bn_vec(dbeta, torch.float32, 64, c, "bn_train_grad_stats", "out[1] (dbeta)")
        _bn_vec(grec, torch.float64, 128, c, "bn_train_grad_stats", "out[2] (grad_record)")
    ws = _bn_ws(workspace, n * H * W, c, "bn_train_grad_stats")
    with _dev(c):
        _check(load().deqsci_bn_train_grad_stats_f32(gy.data_ptr(), c.data_ptr(), rp, float(eps), grec.data_ptr(), dgamma.data_ptr(),
                                                     dbeta.data_ptr(), n * H * W, ws.data_ptr(), _stream()), "bn_train_grad_stats")
    return dgamma, dbeta, grec


def bn_train_grad_apply(gy, c, record, grad_record, gamma, eps, out=None):
    """T4: dc = gamma / sqrt(var + eps) (gy - dbeta / P - xhat dgamma / P), the gradient behind the convolution, statistic terms included
    (they reach the pixels the ReLU masked too); out may be gy.  1 launch."""
    _act64(gy, "bn_train_grad_apply", "gy"), _act64(c, "bn_train_grad_apply", "c")
    if gy.shape != c.shape or gy.device != c.device:
        raise DeqsciHipError(f"bn_train_grad_apply: gy {tuple(gy.shape)} and c {tuple(c.shape)} must have one shape and device")
    n, _, H, W = c.shape
    o = torch.empty_like(gy, memory_format=torch.channels_last) if out is None else out
    if o is not gy:
        _act64(o, "bn_train_grad_apply", "out")
        if o.shape != gy.shape or o.device != gy.device:
            raise DeqsciHipError(f"bn_train_grad_apply: out {tuple(o.shape)} must have gy's shape {tuple(gy.shape)} and device")
    rp = _bn_vec(record, torch.float64, 128, c, "bn_train_grad_apply", "record")
    gr = _bn_vec(grad_record, torch.float64, 128, c, "bn_train_grad_apply", "grad_record")
    gp = _bn_vec(gamma, torch.float32, 64, c, "bn_train_grad_apply", "gamma")
    with _dev(c):
        _check(load().deqsci_bn_train_grad_apply_f32(gy.data_ptr(), c.data_ptr(), rp, gr, gp, float(eps), o.data_ptr(), n * H * W, _stream()),
               "bn_train_grad_apply")
    return o


def conv3x3_c1_to_64_masked(x, w_packed, mask, out=None):
    """x (n,1,H,W) planar -> conv3x3(x, w, pad=1) * mask as a channels_last (n,64,H,W) activation (mask: relu_mask_pack's words)."""
    n, c, H, W = x.shape
    if c != 1:
        raise DeqsciHipError(f"conv3x3_c1_to_64_masked: (n,1,H,W) image required, got {tuple(x.shape)}")
    o = out if out is not None else torch.empty((n, 64, H, W), device=x.device, dtype=torch.float32, memory_format=torch.channels_last)
    with _dev(x):
        _check(load().deqsci_conv3x3_c1_to_64_masked_f32(_p(x, "x"), _p(w_packed, "w_packed"), _mask_ptr(mask, n, H, W, "conv3x3_c1_to_64_masked"),
                                                         o.data_ptr(), n, H, W, _stream()), "conv3x3_c1_to_64_masked")
    return o


def pack_head_weights(w):
    """(64,5,3,3) conv weight -> [ch*9+tap (45)][cout//4 (16)][cout%4 (4)] for deqsci_ffdnet_head_f32."""
    if tuple(w.shape) != (64, 5, 3, 3):
        raise DeqsciHipError(f"ffdnet head expects a (64,5,3,3) weight, got {tuple(w.shape)}")
    return w.detach().float().reshape(16, 4, 45).permute(2, 0, 1).contiguous()


def ffdnet_head(x, w_packed, sigma, out=None):
    """x (n,1,2H,2W) planar, sigma (n,) or (1,) -> relu(conv3x3(cat(sigma map, pixel_unshuffle(x,2)), w)) as a
    channels_last (n,64,H,W) activation.  (In front of a run of split-fp16 layers: ffdnet_head_split16.)"""
    n, c, H2, W2 = x.shape
    if c != 1 or H2 % 2 or W2 % 2:
        raise DeqsciHipError(f"ffdnet_head: (n,1,even,even) image required, got {tuple(x.shape)}")
    if sigma.numel() not in (1, n) or sigma.dtype != torch.float32 or not sigma.is_cuda:
        raise DeqsciHipError("ffdnet_head: sigma must be a fp32 GPU tensor with 1 or n elements")
    H, W = H2 // 2, W2 // 2
    o = out if out is not None else torch.empty((n, 64, H, W), device=x.device, dtype=torch.float32,
                                                  memory_format=torch.channels_last)
    with _dev(x):
        _check(load().deqsci_ffdnet_head_f32(_p(x, "x"), _p(w_packed, "w_packed"), sigma.data_ptr(),
                                             0 if sigma.numel() == 1 else sigma.stride(0), o.data_ptr(), n, H, W, _stream()),
               "ffdnet_head")
    return o


def _check_packed(u_packed, positions, packer):
    """The kernels DMA the whole transformed-weight array by size: a wrong pack (the other kernel's, a slice) would be read out of bounds."""
    if not isinstance(u_packed, torch.Tensor) or u_packed.numel() != 64 * 64 * positions:
        raise DeqsciHipError(f"u_packed must hold 64*64*{positions} floats (the output of _hip.{packer}), got "
                             f"{tuple(getattr(u_packed, 'shape', ()))}")


def pack_winograd_weights(w):
    """(64,64,3,3) conv weight -> U = G g G^T of Winograd F(2x2,3x3) in the kernel's MFMA-lane order
    [cin chunk c (8)][xi (16)][cout half wn (2)][q (4)][i (16)][j (2)][s (2)] with cout = 32 wn + 16 j + i and
    cin = 8 c + 2 q + s, so that LDS staging is a linear copy and a lane's B operands are 16 contiguous bytes."""
    if tuple(w.shape) != (64, 64, 3, 3):
        raise DeqsciHipError(f"winograd conv expects a (64,64,3,3) weight, got {tuple(w.shape)}")
    G = torch.tensor([[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]], dtype=torch.float64, device=w.device)
    U = G @ w.detach().double() @ G.t()                      # (cout, cin, 4, 4)
    U = U.permute(2, 3, 0, 1).reshape(16, 2, 2, 16, 8, 4, 2)  # [xi][wn][j][i][c][q][s]
    return U.permute(4, 0, 1, 5, 3, 2, 6).contiguous().float()   # [c][xi][wn][q][i][j][s]


def conv3x3_c64_winograd(x, u_packed, bias=None, relu=True, out=None, events=None):
    """x (n,64,H,W) channels_last -> relu(conv3x3(x, w, pad=1) + bias) as a new channels_last tensor (Winograd F(2x2,3x3), fp32 MFMA)."""
    n, c, H, W = x.shape
    if c != 64 or not x.is_contiguous(memory_format=torch.channels_last) or x.dtype != torch.float32 or not x.is_cuda:
        raise DeqsciHipError("conv3x3_c64_winograd: fp32 channels_last GPU activation with 64 channels required")
    _check_packed(u_packed, 16, "pack_winograd_weights")
    o = out if out is not None else torch.empty_like(x, memory_format=torch.channels_last)
    ev = _hook_events("f22", n, H, W, events)
    with _dev(x):
        if ev is None:
            _check(load().deqsci_conv3x3_c64_winograd_f32(x.data_ptr(), _p(u_packed, "u_packed"), _p(bias, "bias", True), o.data_ptr(),
                                                          n, H, W, 1 if relu else 0, _stream()), "conv3x3_c64_winograd")
        else:
            _check(load().deqsci_conv3x3_c64_winograd_timed_f32(x.data_ptr(), _p(u_packed, "u_packed"), _p(bias, "bias", True), o.data_ptr(),
                                                                n, H, W, 1 if relu else 0, _stream(), ev[0], ev[1]), "conv3x3_c64_winograd_timed")
    return o


def conv3x3_c64_winograd_masked(x, u_packed, mask, out=None):
    """x (n,64,H,W) channels_last -> conv3x3(x, w, pad=1) * mask (no bias, no ReLU; mask: relu_mask_pack's words) as a new channels_last
    tensor: the Winograd F(2x2,3x3) kernel with the implicit backward's epilogue."""
    n, c, H, W = x.shape
    if c != 64 or not x.is_contiguous(memory_format=torch.channels_last) or x.dtype != torch.float32 or not x.is_cuda:
        raise DeqsciHipError("conv3x3_c64_winograd_masked: fp32 channels_last GPU activation with 64 channels required")
    _check_packed(u_packed, 16, "pack_winograd_weights")
    o = out if out is not None else torch.empty_like(x, memory_format=torch.channels_last)
    with _dev(x):
        _check(load().deqsci_conv3x3_c64_winograd_masked_f32(x.data_ptr(), _p(u_packed, "u_packed"),
                                                             _mask_ptr(mask, n, H, W, "conv3x3_c64_winograd_masked"), o.data_ptr(),
                                                             n, H, W, _stream()), "conv3x3_c64_winograd_masked")
    return o


def pack_winograd44_weights(w):
    """(64,64,3,3) conv weight -> U = G g G^T of Winograd F(4x4,3x3) (6x6 per cout, cin; computed in float64, rounded once) in the
    LDS order of csrc/winograd44.hip: [cin chunk c (8)][s (18)][rg (2)][cgp (2)][q (4)][i (16)][j (2)][ks (2)] with transform
    position (3 rg + s // 6, s % 6), cout = 32 cgp + 16 j + i, cin = 8 c + 2 q + ks."""
    if tuple(w.shape) != (64, 64, 3, 3):
        raise DeqsciHipError(f"winograd conv expects a (64,64,3,3) weight, got {tuple(w.shape)}")
    G = torch.tensor([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6],
                      [0, 0, 1]], dtype=torch.float64, device=w.device)
    U = G @ w.detach().double() @ G.t()                             # (cout, cin, 6, 6)
    U = U.reshape(2, 2, 16, 8, 4, 2, 2, 3, 6)                       # [cgp][j][i][c][q][ks][rg][sr][sc]
    return U.permute(3, 7, 8, 6, 0, 4, 2, 1, 5).contiguous().float()   # [c][sr][sc][rg][cgp][q][i][j][ks]


ACT_NHWC, ACT_BLK32 = 0, 1

# Measurement hook (bench.py): when set, every launch of a 64->64 kernel asks it for a (start, stop) pair of raw hipEvent_t handles -
# hook(kind, n, H, W) -> (ev0, ev1) or None - and the dispatch's own begin / end timestamps are written to them.
CONV64_EVENT_HOOK = None


def _hook_events(kind, n, H, W, events, layers=1):
    """kind "s16stack": one launch that runs `layers` 64->64 layers over n images; the hook is told through its `layers` keyword (a hook
    that does not take it is not asked about those launches)."""
    if events is not None:
        return events
    if CONV64_EVENT_HOOK is not None:
        if layers == 1:
            return CONV64_EVENT_HOOK(kind, n, H, W)
        try:
            return CONV64_EVENT_HOOK(kind, n, H, W, layers=layers)
        except TypeError:
            return None
    return None



class Blk32:
    """An activation (n,64,H,W) in the "blk32" layout of csrc/winograd44.hip: planes of 8 channels, blocks of 32 columns in the
    kernel's staging order - t is (n, 8, H, ceil(W/32), 32, 8) float32.  Only ever exists between two 64->64 layers."""
    __slots__ = ("t", "n", "H", "W")

    def __init__(self, t, n, H, W):
        self.t, self.n, self.H, self.W = t, n, H, W

    is_cuda = property(lambda self: self.t.is_cuda)
    device = property(lambda self: self.t.device)
    shape = property(lambda self: (self.n, 64, self.H, self.W))

    @staticmethod
    def empty(n, H, W, device):
        return Blk32(torch.empty((n, 8, H, -(-W // 32), 32, 8), dtype=torch.float32, device=device), n, H, W)

    @staticmethod
    def _pos():
        m1 = torch.arange(32) + 1
        return 8 * (m1 & 3) + (m1 >> 2) - ((m1 & 3) == 0).long()        # position of column m inside its block

    @staticmethod
    def from_nchw(x):
        """(tests / tools) any (n,64,H,W) tensor -> blk32; padding columns are filled with NaN: the kernel must never read them."""
        n, c, H, W = x.shape
        Wb = -(-W // 32)
        xp = torch.full((n, 64, H, Wb * 32), float("nan"), dtype=torch.float32, device=x.device)
        xp[..., :W] = x
        t = xp.reshape(n, 8, 8, H, Wb, 32).permute(0, 1, 3, 4, 5, 2)      # (n, chunk, H, Wb, m, ch)
        out = torch.empty_like(t.contiguous())
        out[:, :, :, :, Blk32._pos().to(x.device), :] = t
        return Blk32(out.contiguous(), n, H, W)

    def to_nchw(self):
        t = self.t[:, :, :, :, Blk32._pos().to(self.t.device), :]          # back to column order
        x = t.permute(0, 1, 5, 2, 3, 4).reshape(self.n, 64, self.H, -1)
        return x[..., :self.W].contiguous(memory_format=torch.channels_last)


def conv3x3_c64_winograd44(x, u_packed, bias=None, relu=True, out=None, out_blk=False, events=None):
    """x (n,64,H,W) channels_last, or a Blk32 -> relu(conv3x3(x, w, pad=1) + bias) as a new channels_last tensor, or a Blk32 with
    out_blk=True: Winograd F(4x4,3x3), the large-batch kernel.  events: (start, stop) raw hipEvent_t handles (measurement)."""
    if isinstance(x, Blk32):
        n, H, W, xt, in_l = x.n, x.H, x.W, x.t, ACT_BLK32
        if tuple(xt.shape) != (n, 8, H, -(-W // 32), 32, 8) or not xt.is_contiguous():
            raise DeqsciHipError(f"conv3x3_c64_winograd44: malformed Blk32 {tuple(xt.shape)} for (n, H, W) = {(n, H, W)}")
    else:
        n, c, H, W = x.shape
        if c != 64 or not x.is_contiguous(memory_format=torch.channels_last):
            raise DeqsciHipError("conv3x3_c64_winograd44: fp32 channels_last GPU activation with 64 channels required")
        xt, in_l = x, ACT_NHWC
    if xt.dtype != torch.float32 or not xt.is_cuda:
        raise DeqsciHipError("conv3x3_c64_winograd44: fp32 channels_last GPU activation with 64 channels required")
    _check_packed(u_packed, 36, "pack_winograd44_weights")
    if bias is not None and bias.numel() < 64:
        raise DeqsciHipError(f"conv3x3_c64_winograd44: bias must have 64 elements, got {bias.numel()}")
    if out_blk:
        o = out if out is not None else Blk32.empty(n, H, W, xt.device)
        if not isinstance(o, Blk32) or (o.n, o.H, o.W) != (n, H, W) or o.t.device != xt.device or not o.t.is_contiguous():
            raise DeqsciHipError("conv3x3_c64_winograd44: out must be a Blk32 of the input's (n, H, W) on its device")
        ot = o.t
    else:
        o = out if out is not None else torch.empty((n, 64, H, W), dtype=torch.float32, device=xt.device, memory_format=torch.channels_last)
        if (isinstance(o, Blk32) or tuple(o.shape) != (n, 64, H, W) or o.dtype != torch.float32 or o.device != xt.device
                or not o.is_contiguous(memory_format=torch.channels_last)):
            raise DeqsciHipError("conv3x3_c64_winograd44: out must be a fp32 channels_last (n,64,H,W) tensor on the input's device")
        ot = o
    ev = _hook_events("f44", n, H, W, events) or (None, None)
    with _dev(xt):
        _check(load().deqsci_conv3x3_c64_winograd44_layout_f32(xt.data_ptr(), _p(u_packed, "u_packed"), _p(bias, "bias", True), ot.data_ptr(),
                                                               n, H, W, 1 if relu else 0, in_l, ACT_BLK32 if out_blk else ACT_NHWC, _stream(),
                                                               ev[0], ev[1]), "conv3x3_c64_winograd44")
    return o


# ----------------------------------------------------------------------------- split-fp16 direct convolution (csrc/conv_s16.hip)
# An sp16 activation holds the fp16 pieces hi + lo of 2^e x.  fp32 is scale-free, fp16 is not, so e follows the data, PER IMAGE of the
# batch (a measurement's result never depends on what else is in the batch): the RANGE of an activation is (rng, exp) - `rng` a fp32 GPU
# tensor of n elements, rng[i] = max |x| of image i of that activation as a kernel measured it (every kernel that writes or reads the
# activation derives e(i) = act_exp(rng[i]) from those device words: nothing crosses to the host, a captured hipGraph follows its
# inputs), or None: the fixed exponent `exp` for every image.  The mirror of csrc/common.hpp: sp16_act_exp.
SP16_DEFAULT_EXP, SP16_TARGET_EXP, SP16_EXP_LIMIT = 8, 11, 64
SP16_ACT_SCALE = 2.0 ** SP16_DEFAULT_EXP     # the fixed default: 2^8 x suits activations of a few units (|x| < 255.9)


def act_exp(amax):
    """The exponent e the kernels derive from max |x| = amax: 2^e amax in [2^11, 2^12) (a factor 16 below fp16's overflow; an element
    keeps all 22 bits of its split down to 2^-14 of the maximum).  amax zero / subnormal / not finite: the default 8."""
    import math
    import struct
    b = struct.unpack("<I", struct.pack("<f", float(amax)))[0]
    e = (b >> 23) & 0xff
    if e == 0 or e == 255 or math.isnan(float(amax)):
        return SP16_DEFAULT_EXP
    return max(-SP16_EXP_LIMIT, min(SP16_EXP_LIMIT, SP16_TARGET_EXP - (e - 127)))


def _rng(t, n):
    """Device pointer of the range slots of an n-image activation (a contiguous fp32 GPU tensor of n elements), or None."""
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or t.numel() != n or not t.is_contiguous():
        raise DeqsciHipError(f"range slots must be a contiguous fp32 GPU tensor with one element per image ({n}), got "
                             f"{tuple(getattr(t, 'shape', ()))}")
    return t.data_ptr()


def absmax(x, slots):
    """slots[i] = max(slots[i], max |x[i]|) on the device (zero them first), x (n, ...): the ranges of an activation no sp16-writing
    kernel produced."""
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32):
        raise DeqsciHipError("absmax: fp32 GPU tensor required")
    if not (x.is_contiguous() or (x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last))):    # any dense order per image does
        x = x.contiguous()
    n = x.shape[0]
    with _dev(x):
        _check(load().deqsci_absmax_f32(x.data_ptr(), n, x.numel() // n, _rng(slots, n), _stream()), "absmax")
    return slots


class Sp16:
    """An activation (n,64,H,W) in the "sp16" layout of csrc/conv_s16.hip: t is (n, 4, 2, 2, H, W, 8) float16 =
    [cin chunk][piece: hi, lo][8-channel block][H][W][8 channels], holding 2^e x as hi + lo, e from the range (rng, exp) (see above).
    Only exists between 64->64 layers."""
    __slots__ = ("t", "n", "H", "W", "rng", "exp")

    def __init__(self, t, n, H, W, rng=None, exp=SP16_DEFAULT_EXP):
        self.t, self.n, self.H, self.W, self.rng, self.exp = t, n, H, W, rng, exp

    is_cuda = property(lambda self: self.t.is_cuda)
    device = property(lambda self: self.t.device)
    shape = property(lambda self: (self.n, 64, self.H, self.W))

    @staticmethod
    def empty(n, H, W, device):
        return Sp16(torch.empty((n, 4, 2, 2, H, W, 8), dtype=torch.float16, device=device), n, H, W)

    def exponents(self):
        """The exponent of every image (host sync when the ranges are device slots: tests / tools)."""
        return [self.exp] * self.n if self.rng is None else [act_exp(v) for v in self.rng.tolist()]

    def to_nchw(self):
        """(tests / tools) back to an fp32 (n,64,H,W) channels_last tensor: (hi + lo) / 2^e(image), exactly."""
        sc = torch.tensor([2.0 ** (-e) for e in self.exponents()], dtype=torch.float32, device=self.t.device).view(-1, 1, 1, 1, 1, 1)
        v = (self.t[:, :, 0].float() + self.t[:, :, 1].float()) * sc                               # (n, 4, 2, H, W, 8)
        return v.permute(0, 1, 2, 5, 3, 4).reshape(self.n, 64, self.H, self.W).contiguous(memory_format=torch.channels_last)


def to_split16(x, out=None, rng=None, exp=SP16_DEFAULT_EXP):
    """x (n,64,H,W) fp32 channels_last -> Sp16 with the range (rng, exp) (HIP streaming kernel)."""
    n, c, H, W = x.shape
    if c != 64 or not x.is_contiguous(memory_format=torch.channels_last) or x.dtype != torch.float32 or not x.is_cuda:
        raise DeqsciHipError("to_split16: fp32 channels_last GPU activation with 64 channels required")
    o = out if out is not None else Sp16.empty(n, H, W, x.device)
    o.rng, o.exp = rng, int(exp)
    with _dev(x):
        _check(load().deqsci_f32_to_split16(x.data_ptr(), o.t.data_ptr(), n, H, W, _rng(rng, n), o.exp, _stream()), "f32_to_split16")
    return o


def _weight_exp(w):
    """The power of two that puts max |w| into [2^13, 2^14): the lo pieces of every weight that matters are then normal fp16 numbers."""
    import math
    amax = float(w.abs().max())
    return 0 if amax == 0.0 or not math.isfinite(amax) else 13 - math.floor(math.log2(amax))


class Split16Weights:
    """(64,64,3,3) fp32 conv weight as two fp16 pieces of 2^sw w in the LDS order of csrc/conv_s16.hip:
    [cin chunk c (4)][tap (9)][piece: hi, lo (2)][cout group g (2)][lane (64)][j (8)], cout = 32 g + lane % 32, cin = 16 c + 8 (lane // 32) + j."""
    __slots__ = ("packed", "sw")

    def __init__(self, w):
        if tuple(w.shape) != (64, 64, 3, 3):
            raise DeqsciHipError(f"split16 conv expects a (64,64,3,3) weight, got {tuple(w.shape)}")
        w = w.detach().float()
        self.sw = _weight_exp(w)
        ws = w * (2.0 ** self.sw)
        hi = ws.half()
        lo = (ws - hi.float()).half()
        if not bool(torch.isfinite(hi).all()):
            raise DeqsciHipError("split16 weights overflow fp16")
        p = torch.stack((hi, lo), 0)                                   # (hl, cout, cin, ky, kx)
        p = p.reshape(2, 2, 32, 4, 2, 8, 9)                            # [hl][g][m][c][kb][j][tap]
        self.packed = p.permute(3, 6, 0, 1, 4, 2, 5).contiguous()      # [c][tap][hl][g][kb][m][j]  (lane = 32 kb + m)


class TailSplit16Weights:
    """The last layer's (COUT,64,3,3) weight, COUT = 4 (FFDNet) or 1 (SimpleCNN), for the MFMA tail of csrc/conv_s16.hip: the taps go into
    the matrix N dimension - column 32 nt + lane % 32 = COUT tap + cout - as two fp16 pieces of 2^sw w in the order
    [cin chunk c (4)][piece (2)][N tile nt][lane (64)][j (8)], cin = 16 c + 8 (lane // 32) + j; columns >= 9 COUT are zero."""
    __slots__ = ("packed", "cout", "sw")

    def __init__(self, w):
        cout = w.shape[0]
        if tuple(w.shape) != (cout, 64, 3, 3) or cout not in (1, 4):
            raise DeqsciHipError(f"split16 tail expects a (4,64,3,3) or (1,64,3,3) weight, got {tuple(w.shape)}")
        w = w.detach().float()
        self.sw = _weight_exp(w)
        nt = (9 * cout + 31) // 32
        cols = torch.zeros(32 * nt, 64, dtype=torch.float32, device=w.device)             # [col][cin]
        cols[:9 * cout] = (w * 2.0 ** self.sw).permute(2, 3, 0, 1).reshape(9 * cout, 64)  # col = cout_count * tap + cout
        hi = cols.half()
        lo = (cols - hi.float()).half()
        p = torch.stack((hi, lo), 0).reshape(2, nt, 32, 4, 2, 8)                         # [hl][nt][m][c][kb][j]
        self.packed = p.permute(3, 0, 1, 4, 2, 5).contiguous()                           # [c][hl][nt][kb][m][j]  (lane = 32 kb + m)
        self.cout = cout


class HeadSplit16Weights:
    """FFDNet's first-layer (64,5,3,3) weight for the MFMA head of csrc/conv_s16.hip: two fp16 pieces of 2^sw w as
    [k step (3)][piece (2)][cout group g (2)][lane (64)][j (8)], cout = 32 g + lane % 32, k = 16 ks + 8 (lane // 32) + j = 9 ch + tap
    (k >= 45: zero)."""
    __slots__ = ("packed", "sw")

    def __init__(self, w):
        if tuple(w.shape) != (64, 5, 3, 3):
            raise DeqsciHipError(f"split16 head expects a (64,5,3,3) weight, got {tuple(w.shape)}")
        w = w.detach().float()
        self.sw = _weight_exp(w)
        wk = torch.zeros(64, 48, dtype=torch.float32, device=w.device)
        wk[:, :45] = (w * 2.0 ** self.sw).reshape(64, 45)                               # k = 9 ch + tap
        hi = wk.half()
        lo = (wk - hi.float()).half()
        p = torch.stack((hi, lo), 0).reshape(2, 2, 32, 3, 2, 8)                           # [hl][g][m][ks][kb][j]
        self.packed = p.permute(3, 0, 1, 4, 2, 5).contiguous()                           # [ks][hl][g][kb][m][j]


def ffdnet_head_split16(x, weights, sigma, out=None, in_rng=None, in_exp=SP16_DEFAULT_EXP, out_rng=None, out_exp=SP16_DEFAULT_EXP, track=None):
    """x (n,1,2H,2W) planar, sigma (n,) or (1,) -> relu(conv3x3(cat(sigma map, pixel_unshuffle(x,2)), w)) as an Sp16, on the f16 matrix
    cores with the split-fp16 arithmetic (`weights` = HeadSplit16Weights(w)).  in_rng: range slot holding max |x| of the image (the
    kernel adds sigma itself); (out_rng, out_exp): the range of the output; track: a slot that receives max |output|."""
    return _ffdnet_head("ffdnet_head_split16", Sp16, x, weights, sigma, out, in_rng, in_exp, out_rng, out_exp, track)


def _ffdnet_head(what, act, x, weights, sigma, out, in_rng, in_exp, out_rng, out_exp, track=None):
    """ffdnet_head_split16 (act = Sp16) and ffdnet_head_p32 (act = P32): one kernel each, the same arguments but for `track`, which only
    the sp16 form has."""
    n, c, H2, W2 = x.shape
    if c != 1 or H2 % 2 or W2 % 2 or not isinstance(weights, HeadSplit16Weights):
        raise DeqsciHipError(f"{what}: (n,1,even,even) image and HeadSplit16Weights required, got {tuple(x.shape)}")
    if sigma.numel() not in (1, n) or sigma.dtype != torch.float32 or not sigma.is_cuda:
        raise DeqsciHipError(f"{what}: sigma must be a fp32 GPU tensor with 1 or n elements")
    H, W = H2 // 2, W2 // 2
    o = out if out is not None else act.empty(n, H, W, x.device)
    if not isinstance(o, act) or (o.n, o.H, o.W) != (n, H, W):
        raise DeqsciHipError(f"{what}: out must be a {act.__name__} of the output's shape")
    o.rng, o.exp = out_rng, int(out_exp)
    wp = weights.packed if weights.packed.device == x.device else weights.packed.to(x.device)
    args = (_p(x, "x"), wp.data_ptr(), sigma.data_ptr(), 0 if sigma.numel() == 1 else sigma.stride(0), o.t.data_ptr(), n, H, W, weights.sw,
            _rng(in_rng, n), int(in_exp), _rng(out_rng, n), o.exp)
    with _dev(x):
        if act is Sp16:
            _check(load().deqsci_ffdnet_head_split16(*args, _rng(track, n), _stream()), what)
        else:
            _check(load().deqsci_ffdnet_head_p32(*args, _stream()), what)
    return o


def tail_split16(h, weights, out=None):
    """h Sp16 -> the denoiser's last layer on the f16 matrix cores: COUT = 4: planar noise (n,1,2H,2W) = pixel_shuffle(conv3x3(h, w, pad=1), 2)
    (FFDNet); COUT = 1: (n,1,H,W) = conv3x3(h, w, pad=1) (SimpleCNN).  `weights` = TailSplit16Weights(w)."""
    if not isinstance(h, Sp16):
        raise DeqsciHipError("tail_split16: an Sp16 activation and TailSplit16Weights are required")
    return _tail("tail_split16", h, weights, out)


def _tail(what, h, weights, out):
    """tail_split16 (h Sp16) and ffdnet_tail_p32 (h P32): the kernel is picked by h's layout and the weights' COUT."""
    if not isinstance(weights, TailSplit16Weights):
        raise DeqsciHipError(f"{what}: TailSplit16Weights of a (4,64,3,3) or (1,64,3,3) weight are required")
    f = 2 if weights.cout == 4 else 1
    o = out if out is not None else torch.empty((h.n, 1, f * h.H, f * h.W), device=h.t.device, dtype=torch.float32)
    wp = weights.packed if weights.packed.device == h.t.device else weights.packed.to(h.t.device)
    if isinstance(h, Sp16):
        fn = load().deqsci_ffdnet_tail_split16 if weights.cout == 4 else load().deqsci_conv3x3_c64_to_1_split16
    else:
        fn = load().deqsci_ffdnet_tail_p32 if weights.cout == 4 else load().deqsci_conv3x3_c64_to_1_p32
    with _dev(h.t):
        _check(fn(h.t.data_ptr(), wp.data_ptr(), _p(o, "out"), h.n, h.H, h.W, weights.sw, _rng(h.rng, h.n), h.exp, _stream()), what)
    return o


def conv3x3_c64_split16(x, weights, bias=None, relu=True, out=None, out_f32=False, events=None, out_rng=None, out_exp=SP16_DEFAULT_EXP,
                        track=None):
    """x Sp16 -> relu(conv3x3(x, w, pad=1) + bias) as an Sp16 with the range (out_rng, out_exp) (out_f32=False) or an fp32 channels_last
    (n,64,H,W) tensor: the direct convolution on the f16 matrix cores with split operands (csrc/conv_s16.hip).  `weights` =
    Split16Weights(w).  track: a range slot - a MEASURING launch: max |output| is folded into the slot, nothing else is written, None is
    returned (run it, then the real launch with out_rng = that slot)."""
    if not isinstance(x, Sp16) or tuple(x.t.shape) != (x.n, 4, 2, 2, x.H, x.W, 8) or not x.t.is_contiguous() or x.t.dtype != torch.float16 or not x.t.is_cuda:
        raise DeqsciHipError("conv3x3_c64_split16: a contiguous Sp16 GPU activation is required")
    if not isinstance(weights, Split16Weights) or weights.packed.numel() != 4 * 9 * 2 * 2 * 64 * 8:
        raise DeqsciHipError("conv3x3_c64_split16: weights must be a Split16Weights")
    n, H, W, dev = x.n, x.H, x.W, x.t.device
    wp = weights.packed if weights.packed.device == dev else weights.packed.to(dev)
    if track is not None:
        if out_f32:
            raise DeqsciHipError("conv3x3_c64_split16: a measuring launch (track=) serves the sp16 output")
        with _dev(x.t):
            _check(load().deqsci_conv3x3_c64_split16(x.t.data_ptr(), wp.data_ptr(), _p(bias, "bias", True), None, n, H, W, 1 if relu else 0,
                                                     weights.sw, _rng(x.rng, n), x.exp, None, 0, _rng(track, n), 0, _stream(), None, None),
                   "conv3x3_c64_split16 (measuring)")
        return None
    if out_f32:
        o = out if out is not None else torch.empty((n, 64, H, W), dtype=torch.float32, device=dev, memory_format=torch.channels_last)
        ot = o
    else:
        o = out if out is not None else Sp16.empty(n, H, W, dev)
        o.rng, o.exp = out_rng, int(out_exp)
        ot = o.t
    ev = _hook_events("s16", n, H, W, events) or (None, None)
    with _dev(x.t):
        _check(load().deqsci_conv3x3_c64_split16(x.t.data_ptr(), wp.data_ptr(), _p(bias, "bias", True), ot.data_ptr(), n, H, W, 1 if relu else 0,
                                                 weights.sw, _rng(x.rng, n), x.exp, _rng(out_rng, n), int(out_exp), None, 1 if out_f32 else 0,
                                                 _stream(), ev[0], ev[1]), "conv3x3_c64_split16")
    return o


class _Stack:
    """A RUN of 64->64 layers for one stack launch: the device table of (weights, bias, w_exp, relu) per layer - three 8-byte words each -
    the tensors it points to (kept alive here), and per launch shape the progress words of the tiles (zeroed once: they count on from
    launch to launch) and the two ping-pong buffers (kept: a captured hipGraph carries their addresses).  Split16Stack and Wino16Stack
    name their kernel's activation class ACT, weights class WEIGHTS, block TILE (rows x columns of output pixels), measurement hook kind
    HOOK, C entry point ENTRY and launch function (the engine's slice-by-slice f-call; its first and last layer: engine._Edges)."""
    __slots__ = ("table", "n_layers", "keep", "_state")

    def __init__(self, layers, device):
        """layers: [(WEIGHTS, bias tensor or None, relu), ...]"""
        rows, keep = [], []
        for w16, bias, relu in layers:
            if not isinstance(w16, self.WEIGHTS):
                raise DeqsciHipError(f"{type(self).__name__}: every layer needs {self.WEIGHTS.__name__}")
            wp = w16.packed if w16.packed.device == torch.device(device) else w16.packed.to(device)
            b = None if bias is None else f32c(bias.detach().to(device))
            if b is not None and b.numel() < 64:
                raise DeqsciHipError(f"{type(self).__name__}: bias must have 64 elements")
            keep += [wp, b]
            rows += [wp.data_ptr(), 0 if b is None else b.data_ptr(), (int(w16.sw) & 0xffffffff) | ((1 if relu else 0) << 32)]
        self.table = torch.tensor(rows, dtype=torch.int64).to(device)
        self.n_layers, self.keep, self._state = len(layers), keep, {}

    def state(self, n, H, W):
        """(ACT, ACT) ping-pong outputs of a batch of n images (kept: a captured hipGraph carries their addresses)."""
        st = self._state.get(("out", n, H, W))
        if st is None:
            dev = self.table.device
            for key in [k for k in self._state if k[0] == "out"]:      # one live batch shape at a time (2 x 256 bytes per pixel and image)
                del self._state[key]
            st = self._state[("out", n, H, W)] = (self.ACT.empty(n, H, W, dev), self.ACT.empty(n, H, W, dev))
        return st

    def head_buffer(self, n, H, W):
        """An ACT for the run's INPUT of a slice of n images (the engine runs first layer -> run -> last layer slice by slice, so that each
        hands its output to the next through the Infinity Cache); kept like the output buffers."""
        hb = self._state.get(("head", n, H, W))
        if hb is None:
            for key in [k for k in self._state if k[0] == "head"]:
                del self._state[key]
            hb = self._state[("head", n, H, W)] = self.ACT.empty(n, H, W, self.table.device)
        return hb

    def flags(self, n, H, W):
        """The progress words of a LAUNCH of n images: 32 (n_tiles + 1) words (a 128-byte line per tile + the time-out word), zeroed once.
        Launches of one shape share them (they run one after the other on a stream and each advances every word by n_layers)."""
        fl = self._state.get(("flags", n, H, W))
        if fl is None:
            n_tiles = n * (-(-H // self.TILE[0])) * (-(-W // self.TILE[1]))
            fl = self._state[("flags", n, H, W)] = torch.zeros(32 * (n_tiles + 1), dtype=torch.int32, device=self.table.device)
        return fl

    def timed_out(self):
        """(host sync) True if a wait of any launch since the last call timed out - the outputs since then are invalid; the words are
        rearmed."""
        bad = False
        for key, fl in self._state.items():
            if key[0] == "flags" and int(fl[-32]) != 0:
                fl.zero_()
                bad = True
        return bad


STACK_SLICE_BYTES = 128 << 20      # activation bytes of one stack launch: its two ping-pong buffers share the 256 MiB Infinity Cache


def split16_stack_per_launch(n, H, W, slice_bytes=STACK_SLICE_BYTES, cus=None, tile=(16, 32)):
    """Images per stack launch for a batch of n images of H x W: as many as keep one activation (256 bytes per pixel) within `slice_bytes`
    (32 images of 128 x 128) - rounded down to a whole number of 16 x 32 tiles per CU when the device's CU count is given (a launch of
    2.75 tiles per workgroup takes as long as one of 3): a batch goes out as full slices and a remainder (40 images: 32 + 8).  Measured
    on MI355X at 256 x 256 x 8, FFDNet, 8 measurements per call: slices of 32 / 16 images 148 / 147 frames/s, of 22 / 11 images (704 / 352
    tiles on 256 CUs) 140 / 122, of 40-64 images 138-141 (as with a launch per layer)."""
    per = max(1, int(slice_bytes) // (H * W * 256))
    if cus:
        tiles = (-(-H // tile[0])) * (-(-W // tile[1]))
        unit = int(cus) // math.gcd(tiles, int(cus))             # images whose tiles are a multiple of the CUs
        if per >= unit:
            per -= per % unit
    return min(per, n)


def conv3x3_c64_split16_stack(x, stack, ranges=None, events=None, per_launch=None, rng_offset=0, out_bufs=None, check=None):
    """x Sp16 -> the run of 64->64 layers `stack` (Split16Stack), each launch a whole run (csrc/conv_s16.hip, STACK: the persistent
    workgroups walk their tiles layer after layer, a tile waiting for the layer before of itself and its eight neighbours) over a slice
    of the batch - per_launch images (None: split16_stack_per_launch, slices that fit the Infinity Cache), one launch after the other;
    ranges: the (n_layers + 1, n) range slots of the run - its input's first - or None (fixed exponents: the input's, then 2^8).
    Returns the Sp16 the last layer wrote (one of the stack's two buffers of this shape).  stack.timed_out() afterwards tells whether a
    wait gave up (foreign work on the device's CUs): the result is invalid then.  x may itself be a slice of a larger batch: then
    `ranges` are the whole batch's (n_layers + 1, n_total) slots and rng_offset the slice's first image in them; out_bufs: two Sp16 of at
    least x.n images to write into instead of the stack's own."""
    if not isinstance(x, Sp16) or not isinstance(stack, Split16Stack) or not x.t.is_contiguous() or x.t.dtype != torch.float16 or not x.t.is_cuda:
        raise DeqsciHipError("conv3x3_c64_split16_stack: a contiguous Sp16 GPU activation and a Split16Stack are required")
    return _stack_launch("conv3x3_c64_split16_stack", x, stack, ranges, events, per_launch, rng_offset, out_bufs, check)


def _stack_launch(what, x, stack, ranges, events, per_launch, rng_offset, out_bufs, check):
    """conv3x3_c64_split16_stack and conv3x3_c64_wino16_stack once x and the stack's type are checked: the kernel, layout and tile are the
    stack's."""
    n, H, W = x.n, x.H, x.W
    if x.t.device != stack.table.device:
        raise DeqsciHipError(f"{what}: the stack was built for another device")
    n_total = n if ranges is None or not isinstance(ranges, torch.Tensor) or ranges.dim() != 2 else ranges.shape[1]
    if ranges is not None and (not isinstance(ranges, torch.Tensor) or ranges.dtype != torch.float32 or ranges.dim() != 2
                               or ranges.shape[0] != stack.n_layers + 1 or rng_offset < 0 or rng_offset + n > n_total
                               or not ranges.is_contiguous() or ranges.device != x.t.device):
        raise DeqsciHipError(f"{what}: ranges must be a contiguous fp32 ({stack.n_layers + 1}, >= {rng_offset + n}) tensor on the input's device")
    if (ranges is None) != (x.rng is None):
        raise DeqsciHipError(f"{what}: the input's range and the run's ranges go together (both measured or both fixed)")
    per = split16_stack_per_launch(n, H, W, cus=_cus(x.t.device), tile=stack.TILE) if per_launch is None else int(per_launch)
    if per <= 0:
        raise DeqsciHipError(f"{what}: per_launch must be positive")
    bufs = stack.state(n, H, W) if out_bufs is None else out_bufs
    if len(bufs) != 2 or any(type(b) is not stack.ACT or b.n < n or (b.H, b.W) != (H, W) or not b.t.is_contiguous() or b.t.device != x.t.device for b in bufs):
        raise DeqsciHipError(f"{what}: out_bufs must be two contiguous {stack.ACT.__name__} of the input's H x W with at least its images")
    fn = getattr(load(), stack.ENTRY)
    with _dev(x.t):
        for a in range(0, n, per):
            m = min(per, n - a)
            ev = _hook_events(stack.HOOK, m, H, W, events, layers=stack.n_layers) or (None, None)
            _check(fn(x.t[a:a + m].data_ptr(), bufs[0].t[a:a + m].data_ptr(), bufs[1].t[a:a + m].data_ptr(), stack.table.data_ptr(), stack.n_layers,
                      m, H, W, None if ranges is None else ranges.data_ptr() + 4 * (rng_offset + a), n_total, x.exp, SP16_DEFAULT_EXP,
                      stack.flags(m, H, W).data_ptr(), _stream(), ev[0], ev[1]), what)
    out = bufs[(stack.n_layers - 1) % 2]
    if out.n != n:
        out = stack.ACT(out.t[:n], n, H, W)
    out.rng, out.exp = (None if ranges is None else ranges[stack.n_layers][rng_offset:rng_offset + n]), SP16_DEFAULT_EXP
    if check is None:
        check = not torch.cuda.is_current_stream_capturing()
    if check and stack.timed_out():                             # (one host sync; DEQSCIEngine passes check=False and looks once per reconstruction)
        raise DeqsciHipError("a wait inside the stack launch timed out - its workgroups were not all resident (the device's CUs are shared with "
                             "other work): the output of this call is invalid; use one launch per layer")
    return out


class Split16Stack(_Stack):
    """A run of layers of Split16Weights for deqsci_conv3x3_c64_split16_stack (the direct kernel): Sp16 activations."""
    __slots__ = ()
    ACT, WEIGHTS, TILE, HOOK, ENTRY = Sp16, Split16Weights, (16, 32), "s16stack", "deqsci_conv3x3_c64_split16_stack"
    launch = staticmethod(conv3x3_c64_split16_stack)


# ----------------------------------------------------------------------------- split-fp16 Winograd F(2,3) x direct (csrc/conv_w16.hip)

class P32:
    """An activation (n,64,H,W) in the "p32" layout of csrc/conv_w16.hip: t is (n, 8, 2, H, ceil(W/64), 2, 32, 4) float32 =
    [8-channel block][half of 4][H][block of 64 columns][column parity][32][4 channels] holding 2^e x, e from the range (rng, exp) exactly
    as for Sp16 - the 16 planes of 16-byte pixels of sp16, unsplit, and inside every block of 64 columns the even columns first, then the
    odd ones (the Winograd kernel's lanes own column PAIRS: with the parities apart its loads and stores are contiguous).  Columns >= W of
    the last block are padding (never read as data).  Only exists between 64->64 layers."""
    __slots__ = ("t", "n", "H", "W", "rng", "exp")

    def __init__(self, t, n, H, W, rng=None, exp=SP16_DEFAULT_EXP):
        self.t, self.n, self.H, self.W, self.rng, self.exp = t, n, H, W, rng, exp

    is_cuda = property(lambda self: self.t.is_cuda)
    device = property(lambda self: self.t.device)
    shape = property(lambda self: (self.n, 64, self.H, self.W))

    @staticmethod
    def empty(n, H, W, device):
        return P32(torch.empty((n, 8, 2, H, -(-W // 64), 2, 32, 4), dtype=torch.float32, device=device), n, H, W)

    def exponents(self):
        return [self.exp] * self.n if self.rng is None else [act_exp(v) for v in self.rng.tolist()]

    def to_nchw(self):
        """(tests / tools) back to an fp32 (n,64,H,W) channels_last tensor: t / 2^e(image), exactly."""
        sc = torch.tensor([2.0 ** (-e) for e in self.exponents()], dtype=torch.float32, device=self.t.device).view(-1, 1, 1, 1)
        nb = self.t.shape[4]
        v = self.t.permute(0, 1, 2, 7, 3, 4, 6, 5).reshape(self.n, 64, self.H, nb * 64)[..., :self.W]     # (n, b8, j, k, H, blk, i, par) -> col = 64 blk + 2 i + par
        return (v * sc).contiguous(memory_format=torch.channels_last)

    @staticmethod
    def from_nchw(x, rng=None, exp=SP16_DEFAULT_EXP):
        """(tests / tools; torch ops) x (n,64,H,W) fp32 -> P32 holding 2^e x (the padding columns zero)."""
        n, c, H, W = x.shape
        o = P32.empty(n, H, W, x.device)
        o.rng, o.exp = rng, int(exp)
        sc = torch.tensor([2.0 ** e for e in o.exponents()], dtype=torch.float32, device=x.device).view(-1, 1, 1, 1)
        nb = o.t.shape[4]
        xp = torch.zeros((n, 64, H, nb * 64), dtype=torch.float32, device=x.device)
        xp[..., :W] = x * sc
        o.t.copy_(xp.reshape(n, 8, 2, 4, H, nb, 32, 2).permute(0, 1, 2, 4, 5, 7, 6, 3))
        return o


_W16_G = ((1.0, 0.0, 0.0), (0.5, 0.5, 0.5), (0.5, -0.5, 0.5), (0.0, 0.0, 1.0))      # G of Winograd F(2,3)


class Wino16Weights:
    """(64,64,3,3) fp32 conv weight for csrc/conv_w16.hip: U[dy][xi] = sum_dx G[xi][dx] w[:, :, dy, dx] formed in float64, rounded to fp32,
    as two fp16 pieces of 2^sw U (max |U| in [2^13, 2^14)) in the kernel's LDS order
    [cin chunk c (4)][xi half h (2)][xi' (2)][dy (3)][piece: hi, lo (2)][cout group g (2)][lane (64)][j (8)],
    xi = 2 h + xi', cout = 32 g + lane % 32, cin = 16 c + 8 (lane // 32) + j."""
    __slots__ = ("packed", "sw")

    def __init__(self, w):
        if tuple(w.shape) != (64, 64, 3, 3):
            raise DeqsciHipError(f"wino16 conv expects a (64,64,3,3) weight, got {tuple(w.shape)}")
        g = torch.tensor(_W16_G, dtype=torch.float64, device=w.device)
        u = torch.einsum('xk,ocyk->yxoc', g, w.detach().double()).float()           # [dy][xi][cout][cin]
        self.sw = _weight_exp(u)
        us = u * (2.0 ** self.sw)
        hi = us.half()
        lo = (us - hi.float()).half()
        if not bool(torch.isfinite(hi).all()):
            raise DeqsciHipError("wino16 weights overflow fp16")
        p = torch.stack((hi, lo), 0)                                   # (hl, dy, xi, cout, cin)
        p = p.reshape(2, 3, 2, 2, 2, 32, 4, 2, 8)                      # [hl][dy][h][xp][g][m][c][kb][j]
        self.packed = p.permute(6, 2, 3, 1, 0, 4, 7, 5, 8).contiguous()   # [c][h][xp][dy][hl][g][kb][m][j]  (lane = 32 kb + m)


def _act_check(x, what):
    if (not isinstance(x, P32) or tuple(x.t.shape) != (x.n, 8, 2, x.H, -(-x.W // 64), 2, 32, 4) or x.t.dtype != torch.float32 or not x.t.is_contiguous()
            or not x.t.is_cuda):
        raise DeqsciHipError(f"{what}: a contiguous P32 GPU activation is required")


def conv3x3_c64_wino16(x, weights, bias=None, relu=True, out=None, events=None, out_rng=None, out_exp=SP16_DEFAULT_EXP):
    """x P32 -> relu(conv3x3(x, w, pad=1) + bias) as a P32 with the range (out_rng, out_exp): the split-fp16 arithmetic under Winograd F(2,3)
    along x nested in the direct sum along y (csrc/conv_w16.hip).  `weights` = Wino16Weights(w)."""
    _act_check(x, "conv3x3_c64_wino16")
    if not isinstance(weights, Wino16Weights) or weights.packed.numel() != 4 * 2 * 2 * 3 * 2 * 2 * 64 * 8:
        raise DeqsciHipError("conv3x3_c64_wino16: weights must be a Wino16Weights")
    n, H, W, dev = x.n, x.H, x.W, x.t.device
    wp = weights.packed if weights.packed.device == dev else weights.packed.to(dev)
    o = out if out is not None else P32.empty(n, H, W, dev)
    if not isinstance(o, P32):
        raise DeqsciHipError("conv3x3_c64_wino16: out must be a P32")
    o.rng, o.exp = out_rng, int(out_exp)
    ev = _hook_events("w16", n, H, W, events) or (None, None)
    with _dev(x.t):
        _check(load().deqsci_conv3x3_c64_wino16(x.t.data_ptr(), wp.data_ptr(), _p(bias, "bias", True), o.t.data_ptr(), n, H, W, 1 if relu else 0,
                                                weights.sw, _rng(x.rng, n), x.exp, _rng(out_rng, n), int(out_exp), _stream(), ev[0], ev[1]),
               "conv3x3_c64_wino16")
    return o


def ffdnet_head_p32(x, weights, sigma, out=None, in_rng=None, in_exp=SP16_DEFAULT_EXP, out_rng=None, out_exp=SP16_DEFAULT_EXP):
    """ffdnet_head_split16 writing a P32 (the input of a run of conv3x3_c64_wino16 layers): same weights, same arithmetic, 2^e y unsplit."""
    return _ffdnet_head("ffdnet_head_p32", P32, x, weights, sigma, out, in_rng, in_exp, out_rng, out_exp)


def ffdnet_tail_p32(h, weights, out=None):
    """tail_split16 reading a P32: COUT = 4 (FFDNet's last layer + pixel shuffle) or 1 (a plain 64 -> 1 layer: SimpleCNN's last);
    `weights` = TailSplit16Weights(w)."""
    _act_check(h, "ffdnet_tail_p32")
    return _tail("ffdnet_tail_p32", h, weights, out)


def conv3x3_c64_wino16_stack(x, stack, ranges=None, events=None, per_launch=None, rng_offset=0, out_bufs=None, check=None):
    """conv3x3_c64_split16_stack on the Winograd kernel: x P32 -> the run of 64->64 layers `stack` (Wino16Stack), each launch a whole run
    over a slice of the batch; same arguments, same time-out contract."""
    _act_check(x, "conv3x3_c64_wino16_stack")
    if not isinstance(stack, Wino16Stack):
        raise DeqsciHipError("conv3x3_c64_wino16_stack: a Wino16Stack is required")
    return _stack_launch("conv3x3_c64_wino16_stack", x, stack, ranges, events, per_launch, rng_offset, out_bufs, check)


class Wino16Stack(_Stack):
    """A run of layers of Wino16Weights for deqsci_conv3x3_c64_wino16_stack (the Winograd kernel): P32 activations, block tiles of 8 x 64
    pixels."""
    __slots__ = ()
    ACT, WEIGHTS, TILE, HOOK, ENTRY = P32, Wino16Weights, (8, 64), "w16stack", "deqsci_conv3x3_c64_wino16_stack"
    launch = staticmethod(conv3x3_c64_wino16_stack)


class Conv64Weights:
    """The weights of one 64->64 layer for all three kernels.  The split-fp16 pack (a host sync: max |w|) is made here when `s16` is set
    - the engine does whenever its policy can pick that kernel, so that the pack never falls inside a hipGraph capture - or on first use."""
    __slots__ = ("f22", "f44", "_w", "_s16", "_w16")

    def __init__(self, w, s16=False, f22=None, f44=None):
        # f22 / f44: the caller's own pack buffers, which realsn_pack fills on the device (a weight that changes at every f-call)
        self.f22 = pack_winograd_weights(w) if f22 is None else f22
        self.f44 = pack_winograd44_weights(w) if f44 is None else f44
        self._w, self._s16, self._w16 = w.detach(), None, None
        if s16:
            self._s16 = Split16Weights(self._w)
            self._w16 = Wino16Weights(self._w)

    @property
    def w16(self):
        if self._w16 is None:
            self._w16 = Wino16Weights(self._w)
        return self._w16

    @property
    def s16(self):
        if self._s16 is None:
            self._s16 = Split16Weights(self._w)
        return self._s16


def pack_conv64_weights(w, s16=False):
    return Conv64Weights(w, s16=s16)


# launch time of one block tile per CU, us (tools/w44_check.py, tools/s16_check.py; profiles/r02_w44_shapes.jsonl, r03_s16_*): the F(4x4,3x3)
# and the split-fp16 kernels do 2x the pixels of F(2x2,3x3) per tile
_T_TILE_F22, _T_TILE_F44, _T_TILE_S16 = 21.5, 33.5, 29.5


W44_MAX_PIXELS = (0x80000000 - 4096 - 2048 - 16) // 256   # per image, width padded to 32 columns: the F(4x4,3x3) launcher's limit
S16_MAX_PIXELS = (0x80000000 - 4096 - 4096 - 16) // 256   # per image (H * W): the split-fp16 launcher's (csrc/conv_s16.hip: RAW_BIAS + 4096 + 16)
FORCE_CONV64 = None                                     # "f22" / "f44" / "s16": set by the tools for A/B runs (never by the package or the environment); overrides every policy below


_CUS = {}


def _cus(device):
    idx = torch.cuda.current_device() if device is None or getattr(device, "index", None) is None else device.index
    if idx not in _CUS:                                  # (get_device_properties costs tens of microseconds: not once per layer call)
        _CUS[idx] = torch.cuda.get_device_properties(idx).multi_processor_count
    return _CUS[idx]


def conv64_kernel_for(n, H, W, device=None, policy="fast"):
    """'s16', 'f44' or 'f22' for a 64->64 layer on n images of H x W.  All three kernels run one persistent workgroup per CU over
    block tiles of 16 x 16 (F(2x2,3x3)) / 16 x 32 (F(4x4,3x3), split-fp16) output pixels, so a launch takes (waves of block tiles) x
    (time of a tile).
      "fast"    the faster of the split-fp16 direct convolution (csrc/conv_s16.hip) and Winograd F(2x2,3x3) (csrc/winograd.hip): split-fp16
                from about one block tile per CU on (6 images of 128 x 128), F(2x2,3x3) below
      "fast32"  fp32 MFMA arithmetic only: the faster of F(4x4,3x3) (csrc/winograd44.hip) and F(2x2,3x3)
      "f22" / "f44" / "s16"   that kernel whatever the size.
    Rounding per layer against a float64 convolution on FFDNet's own data (tools/conv_error_real.py, profiles/r03_conv_error_real.json):
    split-fp16 1.6e-7, F(2x2,3x3) 2.0e-7, F(4x4,3x3) 2.2e-7 (5.6e-7 on the blocky first iterate), MIOpen's direct fp32 convolution 3.5e-7."""
    if FORCE_CONV64 in ("f22", "f44", "s16"):
        return FORCE_CONV64
    if policy in ("f22", "f44", "s16"):
        return policy
    if policy not in ("fast", "fast32"):
        raise DeqsciHipError(f"conv64 policy {policy!r}: expected 'fast', 'fast32', 'f22', 'f44' or 's16'")
    # beyond the 32-bit buffer offsets of the 16 x 32-tile kernel this policy would pick (its launcher refuses): F(2x2,3x3)
    if (H * (-(-W // 32)) * 32 > W44_MAX_PIXELS) if policy == "fast32" else (H * W > S16_MAX_PIXELS):
        return "f22"
    cus = _cus(device)
    t22 = -(-(n * (-(-H // 16)) * (-(-W // 16))) // cus) * _T_TILE_F22
    big = -(-(n * (-(-H // 16)) * (-(-W // 32))) // cus)
    if policy == "fast32":
        return "f44" if big * _T_TILE_F44 < t22 else "f22"
    return "s16" if big * _T_TILE_S16 < t22 else "f22"


def conv3x3_c64(x, weights, bias=None, relu=True, out=None, policy="fast", chain=False):
    """relu(conv3x3(x, w, pad=1) + bias) for a 64->64 layer on the kernel conv64_kernel_for(..., policy) names (`weights` =
    pack_conv64_weights(w)).  x: fp32 channels_last (n,64,H,W), or the previous layer's output in its kernel's own layout (Sp16 /
    Blk32: that kernel runs again).  chain=True leaves the result in the kernel's own layout for the next 64->64 layer (Sp16 for the
    split-fp16 kernel, Blk32 for F(4x4,3x3); F(2x2,3x3) has none); chain=False returns fp32 channels_last."""
    kind = ("s16" if isinstance(x, Sp16) else "f44" if isinstance(x, Blk32) else
            conv64_kernel_for(x.shape[0], x.shape[2], x.shape[3], x.device, policy))
    if kind == "s16":
        return conv3x3_c64_split16(x if isinstance(x, Sp16) else to_split16(x), weights.s16, bias, relu, out, out_f32=not chain)
    if kind == "f44":
        return conv3x3_c64_winograd44(x, weights.f44, bias, relu, out, out_blk=chain)
    return conv3x3_c64_winograd(x, weights.f22, bias, relu, out)


# ----------------------------------------------------------------------------- evaluation metric (csrc/ssim.hip)
SSIM_MODES = {"same": 0, "valid": 1}


def ssim_window_ok(window):
    return isinstance(window, int) and 3 <= window <= 15 and window % 2 == 1


def ssim_frames(x, y, layout=LAYOUT_HWB, window=11, mode="same", clamp_x=False):
    """Per-frame mean SSIM of x against y (the reference's pytorch_ssim._ssim per frame: Gaussian window, sigma 1.5, zero padding) ->
    (M, B) float64 on the device.  x, y: (M,H,W,B) for LAYOUT_HWB, (M,B,H,W) for LAYOUT_BHW, fp32 on one HIP device.  mode "same" = the
    mean over all H*W map values, "valid" = over the values whose window lies inside the image.  clamp_x: x clamped to [0,1] first.
    The workspace comes from torch's caching allocator; the launches go to the current stream."""
    if tuple(x.shape) != tuple(y.shape) or x.dim() != 4:
        raise DeqsciHipError(f"ssim: x {tuple(x.shape)} and y {tuple(y.shape)} must be the same 4-d shape")
    if mode not in SSIM_MODES:
        raise ValueError(f"ssim mode must be one of {sorted(SSIM_MODES)}, got {mode!r}")
    if not ssim_window_ok(window):
        raise ValueError(f"ssim window must be an odd integer in 3..15, got {window!r}")
    M, H, W, B = _dims(layout, x.shape)
    out = torch.empty((M, B), device=x.device, dtype=torch.float64)
    if M == 0 or B == 0:
        return out
    nbytes = load().deqsci_ssim_workspace_bytes(M, H, W, B, layout)
    if nbytes < 0:
        _check(int(nbytes), "ssim_workspace_bytes")
    ws = torch.empty((max(int(nbytes), 8),), device=x.device, dtype=torch.uint8)
    with _dev(x):
        _check(load().deqsci_ssim_f32(_p(x, "x"), _p(y, "y"), out.data_ptr(), M, H, W, B, layout, window, SSIM_MODES[mode],
                                      1 if clamp_x else 0, ws.data_ptr(), _stream()), "ssim")
    return out


# ----------------------------------------------------------------------------- float64 row sums (csrc/rows.hpp)
def _partials(nbytes, device, given=None, too_small=None):
    """The float64 chunk partials of a *_workspace_bytes query (no initialisation needed): allocated, or the caller's `given`, checked."""
    if given is None:
        return torch.empty((max(int(nbytes) // 8, 1),), device=device, dtype=torch.float64)
    if given.dtype != torch.float64 or given.numel() * 8 < nbytes or given.device != device:
        raise DeqsciHipError(too_small)
    return given


def _same_rows(what, shape, **rows):
    for name, r in rows.items():
        if r is not None and tuple(r.shape) != shape:
            raise DeqsciHipError(f"{what}: {name} {tuple(r.shape)} must be {shape}")


# ----------------------------------------------------------------------------- per-f-call squared error (csrc/trace.hip)
def sqerr_workspace(bsz, N, device):
    """The caller-owned workspace of sqerr_rows for (bsz, N) rows (float64 words; no initialisation needed)."""
    return _partials(load().deqsci_sqerr_workspace_bytes(bsz, N), device)


def sqerr_rows(x, gt, out=None, clamp_x=True, workspace=None):
    """out[s] = sum_i (clamp(x[s, i]) - gt[s, i])^2: difference and square in fp32, the sum in float64 (harness.psnr's arithmetic before
    its mean) -> (bsz,) float64 on the device.  x: (bsz, N) fp32 whose rows are dense but may lie x.stride(0) >= N elements apart (a slot of
    the Anderson history, ws.F[:, slot]); gt: (bsz, N) fp32 contiguous.  clamp_x: x clamped to [0,1] on load.  out / workspace
    (sqerr_workspace): given by a caller that must not allocate (the engine, inside a hipGraph capture); else from torch's allocator."""
    if x.dim() != 2 or tuple(x.shape) != tuple(gt.shape):
        raise DeqsciHipError(f"sqerr_rows: x {tuple(x.shape)} and gt {tuple(gt.shape)} must be the same 2-d shape")
    for name, t in (("x", x), ("gt", gt)):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32):
            raise DeqsciHipError(f"sqerr_rows: {name} must be a float32 tensor on a HIP device; deqsci_amd has no CPU path")
    bsz, N = x.shape
    if not gt.is_contiguous() or (N > 1 and x.stride(1) != 1) or (bsz > 1 and x.stride(0) < N):
        raise DeqsciHipError("sqerr_rows: gt must be contiguous and the rows of x dense")
    if out is None:
        out = torch.empty((bsz,), device=x.device, dtype=torch.float64)
    elif out.dtype != torch.float64 or out.numel() != bsz or not out.is_contiguous() or out.device != x.device:
        raise DeqsciHipError(f"sqerr_rows: out must be {bsz} contiguous float64 values on x's device")
    if bsz == 0 or N == 0:
        return out.zero_()
    workspace = _partials(load().deqsci_sqerr_workspace_bytes(bsz, N), x.device, workspace,
                          "sqerr_rows: workspace too small (sqerr_workspace(bsz, N, device))")
    with _dev(x):
        _check(load().deqsci_sqerr_rows_f32(x.data_ptr(), gt.data_ptr(), out.data_ptr(), bsz, N, x.stride(0) if bsz > 1 else max(x.stride(0), N),
                                            1 if clamp_x else 0, workspace.data_ptr(), _stream()), "sqerr_rows")
    return out


# ----------------------------------------------------------------------------- Jacobian diagnostics (csrc/jacobian.hip)
def pack_head_masked_weights(w):
    """(64,4,3,3) conv weight -> [ch*9+tap (36)][cout//4 (16)][cout%4 (4)] for deqsci_ffdnet_head_masked_f32 (pack_head_weights
    without the sigma channel)."""
    if tuple(w.shape) != (64, 4, 3, 3):
        raise DeqsciHipError(f"ffdnet masked head expects a (64,4,3,3) weight, got {tuple(w.shape)}")
    return w.detach().float().reshape(16, 4, 36).permute(2, 0, 1).contiguous()


def ffdnet_head_masked(x, w_packed, mask, out=None):
    """x (n,1,2H,2W) planar -> conv3x3(pixel_unshuffle(x, 2), w, pad=1) * mask as a channels_last (n,64,H,W) activation (mask:
    relu_mask_pack's words): FFDNet's first layer linearised, or - with the last layer's weight transposed - its last layer's transpose."""
    n, c, H2, W2 = x.shape
    if c != 1 or H2 % 2 or W2 % 2:
        raise DeqsciHipError(f"ffdnet_head_masked: (n,1,even,even) image required, got {tuple(x.shape)}")
    if not isinstance(w_packed, torch.Tensor) or w_packed.numel() != 36 * 64:
        raise DeqsciHipError("ffdnet_head_masked: w_packed must hold 36*64 floats (the output of _hip.pack_head_masked_weights)")
    H, W = H2 // 2, W2 // 2
    o = out if out is not None else torch.empty((n, 64, H, W), device=x.device, dtype=torch.float32, memory_format=torch.channels_last)
    with _dev(x):
        _check(load().deqsci_ffdnet_head_masked_f32(_p(x, "x"), _p(w_packed, "w_packed"), _mask_ptr(mask, n, H, W, "ffdnet_head_masked"),
                                                    o.data_ptr(), n, H, W, _stream()), "ffdnet_head_masked")
    return o


def power_workspace(bsz, N, device):
    """The caller-owned workspace of power_step for (bsz, N) rows (float64 words; no initialisation needed)."""
    return _partials(load().deqsci_power_workspace_bytes(bsz, N), device)


def power_step(w, v_prev, v_out, table_row, workspace=None):
    """One step of a power iteration per sample (row) of w (bsz,N): table_row[s] = (|w_s|^2, <v_prev_s, w_s>) in float64 and
    v_out_s = w_s / |w_s| - zeros, and NaN in the table, where |w_s|^2 is zero or not finite.  v_prev: None (the second entry is NaN) or
    (bsz,N); v_out may be w or v_prev; table_row: (bsz,2) float64 on the device.  No allocation when the workspace (power_workspace) is
    given, no host synchronisation."""
    if w.dim() != 2:
        raise DeqsciHipError(f"power_step: w must be (bsz,N), got {tuple(w.shape)}")
    bsz, N = w.shape
    for name, t in (("v_prev", v_prev), ("v_out", v_out)):
        if t is not None and tuple(t.shape) != (bsz, N):
            raise DeqsciHipError(f"power_step: {name} {tuple(t.shape)} must have w's shape {(bsz, N)}")
    if (not isinstance(table_row, torch.Tensor) or table_row.dtype != torch.float64 or tuple(table_row.shape) != (bsz, 2)
            or not table_row.is_contiguous() or table_row.device != w.device):
        raise DeqsciHipError(f"power_step: table_row must be a contiguous float64 ({bsz},2) tensor on w's device")
    workspace = _partials(load().deqsci_power_workspace_bytes(bsz, N), w.device, workspace,
                          "power_step: workspace too small (power_workspace(bsz, N, device))")
    with _dev(w):
        _check(load().deqsci_power_step_f32(_p(w, "w"), _p(v_prev, "v_prev", True), _p(v_out, "v_out"), table_row.data_ptr(), bsz, N,
                                            workspace.data_ptr(), _stream()), "power_step")
    return v_out


# ----------------------------------------------------------------------------- RealSN in train mode (csrc/realsn.hip)
def _realsn_dims(W, u, what):
    if W.dim() != 4 or tuple(W.shape[2:]) != (3, 3):
        raise DeqsciHipError(f"{what}: weight must be (C_out, C_in, 3, 3), got {tuple(W.shape)}")
    cout, cin = int(W.shape[0]), int(W.shape[1])
    if u.dim() != 4 or u.shape[0] != 1 or u.shape[1] != cout:
        raise DeqsciHipError(f"{what}: u must be (1, {cout}, h, w), got {tuple(u.shape)}")
    return cin, cout, int(u.shape[2]), int(u.shape[3])


def realsn_workspace(cin, cout, h, w, device):
    """The caller-owned workspace of realsn_power / realsn_grad for a (cout, cin, 3, 3) weight and an (h, w) map (no initialisation
    needed); a DeqsciHipError for the sizes the kernels refuse."""
    nbytes = load().deqsci_realsn_workspace_bytes(cin, cout, h, w)
    if nbytes == 0:
        raise DeqsciHipError(f"realsn: no kernel for a ({cout},{cin},3,3) weight on a ({h},{w}) map: (C_in, C_out) must be (1,64), (64,64) "
                             "or (64,1), and h * w at most 2^20")
    return _partials(nbytes, device)


def realsn_power(W, u, n_iters=1, sigma=1.0, eps=1e-12, workspace=None, weight=None, v=None, record=None):
    """n_iters power-iteration steps of a spectrally normalised 3x3 convolution (conv_sn_chen.py:29-50 in the reference) and the
    normalised weight, R1 of csrc/realsn.hip: u (1, C_out, h, w) is read and OVERWRITTEN with the new left vector.
    -> (weight = W / cur_sigma * sigma, u, v (1, C_in, h, w), record): record = float64 (|W^T u|, |W v|, cur_sigma) of the last
    iteration, on the device.  3 n_iters + 1 launches, no host synchronisation.  weight / v / record: the caller's own buffers to write
    (a module's `weight` buffer, in place); with all three and the workspace given the call allocates nothing."""
    cin, cout, h, w = _realsn_dims(W, u, "realsn_power")
    if int(n_iters) < 1:
        raise DeqsciHipError(f"realsn_power: n_iters must be at least 1, got {n_iters}")
    ws = realsn_workspace(cin, cout, h, w, W.device) if workspace is None else workspace
    v = torch.empty((1, cin, h, w), device=W.device, dtype=torch.float32) if v is None else v
    weight = torch.empty_like(W) if weight is None else weight
    record = torch.empty((3,), device=W.device, dtype=torch.float64) if record is None else record
    if tuple(weight.shape) != tuple(W.shape) or v.numel() != cin * h * w or record.dtype != torch.float64 or record.numel() != 3 \
            or not record.is_contiguous() or record.device != W.device:
        raise DeqsciHipError(f"realsn_power: weight must have W's shape {tuple(W.shape)}, v {cin * h * w} elements, record 3 float64 on W's device")
    _p(v, "v")
    with _dev(W):
        _check(load().deqsci_realsn_power_f32(_p(W, "W"), _p(u, "u"), v.data_ptr(), _p(weight, "weight"), record.data_ptr(), int(n_iters),
                                              float(sigma), float(eps), cin, cout, h, w, ws.data_ptr(), _stream()), "realsn_power")
    return weight, u, v, record


def realsn_grad(G, W, u, v, record, sigma=1.0, workspace=None):
    """dL/dW of weight = W / cur_sigma * sigma with cur_sigma = sum(u * (W v)), u and v constants (R2 of csrc/realsn.hip): G = dL/dweight,
    u, v, record as realsn_power left them.  2 launches, no host synchronisation."""
    cin, cout, h, w = _realsn_dims(W, u, "realsn_grad")
    if tuple(G.shape) != tuple(W.shape) or tuple(v.shape) != (1, cin, h, w):
        raise DeqsciHipError(f"realsn_grad: G {tuple(G.shape)} must have W's shape {tuple(W.shape)} and v {tuple(v.shape)} be {(1, cin, h, w)}")
    if record.dtype != torch.float64 or record.numel() != 3 or not record.is_contiguous() or record.device != W.device:
        raise DeqsciHipError("realsn_grad: record must be realsn_power's 3 float64 values on W's device")
    ws = realsn_workspace(cin, cout, h, w, W.device) if workspace is None else workspace
    dW = torch.empty_like(W)
    with _dev(W):
        _check(load().deqsci_realsn_grad_f32(_p(G, "G"), _p(W, "W"), _p(u, "u"), _p(v, "v"), record.data_ptr(), _p(dW, "dW"), float(sigma),
                                             cin, cout, h, w, ws.data_ptr(), _stream()), "realsn_grad")
    return dW


# the shapes of the host packers' outputs: pack_winograd_weights, pack_winograd44_weights, pack_c1_to_64_weights, pack_c64_to_1_weights
_PACK_F22, _PACK_F44, _PACK_WIDE, _PACK_NARROW = (8, 16, 2, 4, 16, 2, 2), (8, 3, 6, 2, 2, 4, 16, 2, 2), (9, 16, 4), (2, 9, 32)


def realsn_pack_shapes(cin, cout):
    """{"pack", "pack44", "pack_t"} -> the shape of each pack realsn_pack writes for a (cout, cin, 3, 3) weight (pack44: None for an
    edge layer) - the shapes of the host packers' own outputs."""
    if (cin, cout) == (64, 64):
        return {"pack": _PACK_F22, "pack44": _PACK_F44, "pack_t": _PACK_F22}
    if (cin, cout) == (1, 64):
        return {"pack": _PACK_WIDE, "pack44": None, "pack_t": _PACK_NARROW}
    if (cin, cout) == (64, 1):
        return {"pack": _PACK_NARROW, "pack44": None, "pack_t": _PACK_WIDE}
    raise DeqsciHipError(f"realsn_pack: no kernel for a ({cout},{cin},3,3) weight: (C_in, C_out) must be (1,64), (64,64) or (64,1)")


def realsn_pack_buffers(cin, cout, device, pack=True, pack44=True, pack_t=True):
    """(pack, pack44, pack_t): the caller-owned buffers of realsn_pack for a (cout, cin, 3, 3) weight, uninitialised; None for a pack that
    is not wanted or does not exist."""
    shapes = realsn_pack_shapes(cin, cout)
    return tuple(torch.empty(shapes[k], device=device, dtype=torch.float32) if want and shapes[k] is not None else None
                 for k, want in (("pack", pack), ("pack44", pack44), ("pack_t", pack_t)))


def realsn_pack(weight, pack=None, pack44=None, pack_t=None):
    """R3 of csrc/realsn.hip: the (cout, cin, 3, 3) weight realsn_power wrote -> the packs the convolution kernels read, written into the
    caller's buffers (realsn_pack_buffers; None: not wanted) by ONE launch with no host synchronisation, host -> device copy or allocation.
    (64,64): pack = pack_winograd_weights(w), pack44 = pack_winograd44_weights(w), pack_t = pack_winograd_weights(vjp._transposed(w)) - U =
    G g G^T in float64 in the one order include/deqsci_hip.h states, rounded once, so equal to the host packers up to that last rounding.
    (1,64): pack = pack_c1_to_64_weights(w), pack_t = pack_c64_to_1_weights(_transposed(w)); (64,1): pack = pack_c64_to_1_weights(w),
    pack_t = pack_c1_to_64_weights(_transposed(w)) - bit for bit.  -> (pack, pack44, pack_t)."""
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3):
        raise DeqsciHipError(f"realsn_pack: weight must be (C_out, C_in, 3, 3), got {tuple(weight.shape)}")
    cout, cin = int(weight.shape[0]), int(weight.shape[1])
    shapes = realsn_pack_shapes(cin, cout)
    for name, t in (("pack", pack), ("pack44", pack44), ("pack_t", pack_t)):
        if t is not None and (shapes[name] is None or t.numel() != math.prod(shapes[name]) or t.device != weight.device):
            raise DeqsciHipError(f"realsn_pack: {name} must hold {shapes[name]} floats on the weight's device, got {tuple(t.shape)} on {t.device}")
    with _dev(weight):
        _check(load().deqsci_realsn_pack_f32(_p(weight, "weight"), _p(pack, "pack", True), _p(pack44, "pack44", True), _p(pack_t, "pack_t", True),
                                             cin, cout, _stream()), "realsn_pack")
    return pack, pack44, pack_t


# ----------------------------------------------------------------------------- Broyden (csrc/broyden.hip)
BROYDEN_MAX_L = 27
BROYDEN_TABLE_STRIDE = 84
# columns of BroydenWorkspace.table: a_j = <dx, U_j>, b_j = <V_j, dg>, c_j = <V_j, gx_new> at A + j, B + j, C + j; |gx_new|^2, d, c_new
BROYDEN_A, BROYDEN_B, BROYDEN_C, BROYDEN_GG, BROYDEN_D, BROYDEN_CNEW = 0, 27, 54, 81, 82, 83


def broyden_chunk():
    """Elements of a row that one workgroup of the Broyden kernels sums (the first stage of their two-stage sums)."""
    return int(load().deqsci_broyden_chunk())


class BroydenWorkspace:
    """Caller-owned buffers of the Broyden step kernels: the planar history U, V (bsz, L, N), the float64 table (bsz, 84) and the chunk
    partials (the library never allocates)."""

    def __init__(self, bsz, N, L, device):
        if not 1 <= L <= BROYDEN_MAX_L:
            raise DeqsciHipError(f"Broyden history L={L} must lie in 1..{BROYDEN_MAX_L}")
        nbytes = int(load().deqsci_broyden_workspace_bytes(bsz, N, L))
        if nbytes == 0:
            raise DeqsciHipError(f"Broyden workspace: unsupported sizes bsz={bsz}, N={N}, L={L}")
        self.bsz, self.N, self.L = bsz, N, L
        self.U = torch.zeros((bsz, L, N), device=device, dtype=torch.float32)
        self.V = torch.zeros((bsz, L, N), device=device, dtype=torch.float32)
        self.table = torch.zeros((bsz, BROYDEN_TABLE_STRIDE), device=device, dtype=torch.float64)
        self.partials = _partials(nbytes, device)


def broyden_dots(ws, dx, gx_old, gx_new, t):
    """ws.table[s] <- a_j, b_j, c_j (j < t) and |gx_new_s|^2 in float64 (two launches, no host synchronisation)."""
    _same_rows("broyden_dots", (ws.bsz, ws.N), dx=dx, gx_old=gx_old, gx_new=gx_new)
    with _dev(ws.U):
        _check(load().deqsci_broyden_dots_f32(_p(ws.U), _p(ws.V), _p(dx, "dx"), _p(gx_old, "gx_old"), _p(gx_new, "gx_new"), ws.table.data_ptr(),
                                              ws.partials.data_ptr(), ws.bsz, ws.N, ws.L, int(t), _stream()), "broyden_dots")


def broyden_update(ws, dx, gx_old, gx_new, t, slot, update, x=None, x_next=None):
    """After broyden_dots with the same rows: the rank-one update into row `slot` of ws.U / ws.V, update = gx_new - sum_j c_j U_j and
    x_next = x + update when given (two launches, no host synchronisation).  update may be dx."""
    _same_rows("broyden_update", (ws.bsz, ws.N), dx=dx, gx_old=gx_old, gx_new=gx_new, update=update, x=x, x_next=x_next)
    with _dev(ws.U):
        _check(load().deqsci_broyden_update_f32(_p(ws.U), _p(ws.V), _p(dx, "dx"), _p(gx_old, "gx_old"), _p(gx_new, "gx_new"), _p(x, "x", True),
                                                _p(x_next, "x_next", True), _p(update, "update"), ws.table.data_ptr(), ws.partials.data_ptr(),
                                                ws.bsz, ws.N, ws.L, int(t), int(slot), _stream()), "broyden_update")
    return update


# ----------------------------------------------------------------------------- the epsilon-algorithm (csrc/epsilon2.hip)
EPSILON2_TABLE_STRIDE = 5
# columns of Epsilon2Workspace.table: sum dx^2, sum df^2, sum d2^2 (without lam), sum (x_new - x)^2, sum x_new^2
EPSILON2_A, EPSILON2_B, EPSILON2_C, EPSILON2_STEP, EPSILON2_NEW = 0, 1, 2, 3, 4


def epsilon2_chunk():
    """Elements of a row that one workgroup of the epsilon2 kernels sums (the first stage of their two-stage sums)."""
    return int(load().deqsci_epsilon2_chunk())


class Epsilon2Workspace:
    """Caller-owned buffers of the epsilon2 step kernels: the float64 table (bsz, 5) and the chunk partials (the library never
    allocates)."""

    def __init__(self, bsz, N, device):
        nbytes = int(load().deqsci_epsilon2_workspace_bytes(bsz, N))
        if nbytes == 0:
            raise DeqsciHipError(f"epsilon2 workspace: unsupported sizes bsz={bsz}, N={N}")
        self.bsz, self.N = bsz, N
        self.table = torch.zeros((bsz, EPSILON2_TABLE_STRIDE), device=device, dtype=torch.float64)
        self.partials = _partials(nbytes, device)


def epsilon2_norms(ws, x, f_x, f_fx):
    """ws.table[s, 0:3] <- the squared norms of dx = f_x - x, df = f_fx - f_x, d2 = df - dx (fp32 differences, float64 sums; two
    launches, no host synchronisation)."""
    _same_rows("epsilon2_norms", (ws.bsz, ws.N), x=x, f_x=f_x, f_fx=f_fx)
    with _dev(x):
        _check(load().deqsci_epsilon2_norms_f32(_p(x, "x"), _p(f_x, "f_x"), _p(f_fx, "f_fx"), ws.table.data_ptr(), ws.partials.data_ptr(),
                                                ws.bsz, ws.N, _stream()), "epsilon2_norms")


def epsilon2_update(ws, x, f_x, f_fx, x_new, lam):
    """After epsilon2_norms with the same rows: x_new = f_x + (df a - dx b) / (c + lam) in fp32 and ws.table[s, 3:5] <- the squared norms
    of x_new - x and x_new (two launches, no host synchronisation).  x_new may overlap none of the inputs."""
    _same_rows("epsilon2_update", (ws.bsz, ws.N), x=x, f_x=f_x, f_fx=f_fx, x_new=x_new)
    with _dev(x):
        _check(load().deqsci_epsilon2_update_f32(_p(x, "x"), _p(f_x, "f_x"), _p(f_fx, "f_fx"), _p(x_new, "x_new"), ws.table.data_ptr(),
                                                 ws.partials.data_ptr(), ws.bsz, ws.N, float(lam), _stream()), "epsilon2_update")
    return x_new


# ----------------------------------------------------------------------------- GAP-TV (csrc/tv.hip)
def _stop_buffer(shape, device, want):
    return torch.empty(shape, device=device, dtype=torch.int32) if want else None


def gaptv(y, phi, phi_sum, maxiter=40, step=1.0, weight=0.3, eps=2e-4, n_iter_max=30, return_stop=False):
    """The reference's GAP_TV_rec per measurement with skimage 0.17.2's denoise_tv_chambolle (multichannel, tau 1/6): y (bsz,H,W),
    Phi (bsz,H,W,B) or (1,H,W,B) (shared), Phi_sum (bsz,H,W) or (1,H,W), fp32 on one HIP device -> (bsz,H,W,B) fp32, and with
    return_stop=True also the (bsz, maxiter, B) int32 stop indices (n_iter_max where the early stop never fired).  State in fp64; the
    launches go to the current stream, the workspace comes from torch's caching allocator."""
    if y.dim() != 3 or phi.dim() != 4 or phi_sum.dim() != 3:
        raise DeqsciHipError(f"gaptv: y (bsz,H,W), Phi (bsz,H,W,B), Phi_sum (bsz,H,W) expected, got {tuple(y.shape)}, "
                             f"{tuple(phi.shape)}, {tuple(phi_sum.shape)}")
    bsz, H, W = y.shape
    B = phi.shape[-1]
    if phi.shape[0] != phi_sum.shape[0] and min(phi.shape[0], phi_sum.shape[0]) == 1:     # one shared, the other per measurement
        phi, phi_sum = phi.expand(bsz, -1, -1, -1).contiguous(), phi_sum.expand(bsz, -1, -1).contiguous()
    shared = _phi_shared(phi, bsz)
    if tuple(phi.shape[1:3]) != (H, W) or tuple(phi_sum.shape[1:]) != (H, W) or phi_sum.shape[0] != phi.shape[0]:
        raise DeqsciHipError(f"gaptv: y {tuple(y.shape)}, Phi {tuple(phi.shape)} and Phi_sum {tuple(phi_sum.shape)} do not match")
    if not isinstance(maxiter, int) or maxiter < 0 or not isinstance(n_iter_max, int) or n_iter_max < 1:
        raise DeqsciHipError(f"gaptv: maxiter >= 0 and n_iter_max >= 1 must be integers, got {maxiter!r}, {n_iter_max!r}")
    out = torch.empty((bsz, H, W, B), device=y.device, dtype=torch.float32)
    stop = _stop_buffer((bsz, maxiter, B), y.device, return_stop)
    nbytes = int(load().deqsci_gaptv_workspace_bytes(bsz, H, W, B))
    _check(min(nbytes, 0), "gaptv_workspace_bytes")
    with _dev(y):
        ws = torch.empty((max(nbytes, 16),), device=y.device, dtype=torch.uint8)
        _check(load().deqsci_gaptv_f32(_p(y, "y"), _p(phi, "Phi"), _p(phi_sum, "Phi_sum"), out.data_ptr(), bsz, H, W, B, shared, maxiter,
                                       float(step), float(weight), float(eps), n_iter_max, None if stop is None else stop.data_ptr(),
                                       ws.data_ptr(), _stream()), "gaptv")
    return (out, stop) if return_stop else out


def tv_chambolle(image, weight=0.1, eps=2e-4, n_iter_max=200, tau=0.25, return_stop=False):
    """skimage 0.17.2's _denoise_tv_chambolle_nd on every plane of image (n,H,W) fp32 on a HIP device, with an explicit tau (1/4 for
    a 2-D array, 1/6 for a (1,H,W) one) -> (n,H,W) fp32 (fp64 inside), and with return_stop=True also the (n,) int32 stop indices."""
    if image.dim() != 3:
        raise DeqsciHipError(f"tv_chambolle: image must be (n,H,W), got {tuple(image.shape)}")
    n, H, W = image.shape
    out = torch.empty((n, H, W), device=image.device, dtype=torch.float32)
    stop = _stop_buffer((n,), image.device, return_stop)
    nbytes = int(load().deqsci_tv_chambolle_workspace_bytes(n, H, W))
    _check(min(nbytes, 0), "tv_chambolle_workspace_bytes")
    with _dev(image):
        ws = torch.empty((max(nbytes, 16),), device=image.device, dtype=torch.uint8)
        _check(load().deqsci_tv_chambolle_f32(_p(image, "image"), out.data_ptr(), n, H, W, float(weight), float(eps), int(n_iter_max),
                                              float(tau), None if stop is None else stop.data_ptr(), ws.data_ptr(), _stream()),
               "tv_chambolle")
    return (out, stop) if return_stop else out


# ----------------------------------------------------------------------------- the training step's glue (csrc/train.hip)
TRAIN_CHUNK = 4096           # DEQSCI_TRAIN_CHUNK: the elements of a workgroup of csrc/train.hip
ADAM_MAX_TENSORS = 64        # DEQSCI_ADAM_MAX_TENSORS: the tensors of one deqsci_adam_step_f32 launch


class AdamEntry(ctypes.Structure):
    """deqsci_adam_entry"""
    _fields_ = [("param", _ptr), ("grad", _ptr), ("exp_avg", _ptr), ("exp_avg_sq", _ptr), ("numel", _i64), ("bc2s", _f32), ("step_size", _f32)]


def mse_workspace(total, device):
    """The caller-owned workspace of mse_stats_grad for `total` elements (float64 words; no initialisation needed)."""
    return _partials(load().deqsci_mse_workspace_bytes(total), device)


def mse_stats_grad(rec, gt, workspace=None, grad=None, stats=None):
    """L1: the loss gradient and the statistics of a training step in one pass -> (grad, stats).  rec, gt: fp32 tensors of one shape on
    the device, dense in the same layout (contiguous; a view into a larger buffer will do - 4-byte alignment is enough).  grad =
    (rec - gt) * (float)(2 / total) in rec's shape; stats (3,) float64 on the device: sum (rec - gt)^2, sum (clamp(rec, 0, 1) - gt)^2 (squares
    in fp32, sums in float64, csrc/rows.hpp's order: deterministic), the number of non-finite differences.  The loss is stats[0] / total,
    the batch PSNR 10 log10(total / stats[1]).  No host synchronisation; workspace / grad / stats: given by a caller that must not allocate."""
    for name, t in (("rec", rec), ("gt", gt)):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32):
            raise DeqsciHipError(f"mse_stats_grad: {name} must be a float32 tensor on a HIP device; deqsci_amd has no CPU path")
    if tuple(rec.shape) != tuple(gt.shape) or not rec.is_contiguous() or not gt.is_contiguous() or rec.device != gt.device:
        raise DeqsciHipError(f"mse_stats_grad: rec {tuple(rec.shape)} and gt {tuple(gt.shape)} must be contiguous, of one shape, on one device")
    total = rec.numel()
    if total == 0:
        raise DeqsciHipError("mse_stats_grad: empty tensors have no mean squared error")
    if grad is None:
        grad = torch.empty_like(rec)
    elif grad.dtype != torch.float32 or tuple(grad.shape) != tuple(rec.shape) or not grad.is_contiguous() or grad.device != rec.device:
        raise DeqsciHipError("mse_stats_grad: grad must be a contiguous float32 tensor of rec's shape on rec's device")
    if stats is None:
        stats = torch.empty((3,), device=rec.device, dtype=torch.float64)
    elif stats.dtype != torch.float64 or stats.numel() != 3 or not stats.is_contiguous() or stats.device != rec.device:
        raise DeqsciHipError("mse_stats_grad: stats must be 3 contiguous float64 values on rec's device")
    workspace = _partials(load().deqsci_mse_workspace_bytes(total), rec.device, workspace,
                          "mse_stats_grad: workspace too small (mse_workspace(total, device))")
    with _dev(rec):
        _check(load().deqsci_mse_stats_grad_f32(rec.data_ptr(), gt.data_ptr(), grad.data_ptr(), stats.data_ptr(), total,
                                                ctypes.c_float(2.0 / total), workspace.data_ptr(), _stream()), "mse_stats_grad")
    return grad, stats


def adam_scalars(step, lr, betas):
    """(bc2s, step_size) of step `step` >= 1 as L2 takes them: sqrt(1 - beta2^t) and lr / (1 - beta1^t), in double."""
    b1, b2 = betas
    return math.sqrt(1.0 - b2 ** step), lr / (1.0 - b1 ** step)


def adam_step(params, grads, exp_avgs, exp_avg_sqs, step, lr, betas, eps, stats=None):
    """L2: one Adam step (torch-1.9 F.adam, no weight decay, no amsgrad) of the listed tensors, ADAM_MAX_TENSORS per launch -> the number of
    launches.  params, exp_avgs, exp_avg_sqs are updated IN PLACE through raw pointers (the caller bumps the parameters' version
    counters); all fp32 on one device, dense (contiguous; views into a flat buffer will do).  step: the step count being taken (>= 1),
    one int or one per tensor.  Builds the table on the host each call: no device allocation, no synchronisation.
    stats: grad_norm's words on the parameters' device - L2c: the step on g * stats[1], and nothing written where stats[2] > 0."""
    n = len(params)
    if not (len(grads) == len(exp_avgs) == len(exp_avg_sqs) == n):
        raise DeqsciHipError("adam_step: params, grads, exp_avgs and exp_avg_sqs must have one length")
    if n == 0:
        return 0
    steps = [int(step)] * n if not isinstance(step, (list, tuple)) else [int(s) for s in step]
    if len(steps) != n or min(steps) < 1:
        raise DeqsciHipError("adam_step: step must be >= 1, one value or one per tensor")
    dev = params[0].device
    for i, quad in enumerate(zip(params, grads, exp_avgs, exp_avg_sqs)):
        for name, t in zip(("param", "grad", "exp_avg", "exp_avg_sq"), quad):
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.device == dev
                    and t.numel() == quad[0].numel() and t.numel() > 0):
                raise DeqsciHipError(f"adam_step: {name} {i} must be a non-empty contiguous float32 tensor of the parameter's size on {dev}")
    if stats is not None and not (isinstance(stats, torch.Tensor) and stats.dtype == torch.float64 and stats.device == dev and stats.is_contiguous()
                                  and stats.numel() >= 3):
        raise DeqsciHipError(f"adam_step: stats must be at least 3 contiguous float64 values on {dev} (grad_norm's)")
    b1, b2 = float(betas[0]), float(betas[1])
    lib, launches = load(), 0
    scalars = {}
    with _dev(params[0]):
        st = _stream()
        for lo in range(0, n, ADAM_MAX_TENSORS):
            hi = min(n, lo + ADAM_MAX_TENSORS)
            table = (AdamEntry * (hi - lo))()
            for j in range(lo, hi):
                t = steps[j]
                if t not in scalars:
                    scalars[t] = adam_scalars(t, float(lr), (b1, b2))
                e = table[j - lo]
                e.param, e.grad, e.exp_avg, e.exp_avg_sq = params[j].data_ptr(), grads[j].data_ptr(), exp_avgs[j].data_ptr(), exp_avg_sqs[j].data_ptr()
                e.numel = params[j].numel()
                e.bc2s, e.step_size = scalars[t]
            if stats is None:
                _check(lib.deqsci_adam_step_f32(ctypes.cast(table, _ptr), hi - lo, b1, 1.0 - b1, b2, 1.0 - b2, float(eps), st), "adam_step")
            else:
                _check(lib.deqsci_adam_step_clipped_f32(ctypes.cast(table, _ptr), hi - lo, b1, 1.0 - b1, b2, 1.0 - b2, float(eps),
                                                        stats.data_ptr(), st), "adam_step (clipped)")
            launches += 1
    return launches


class GradEntry(ctypes.Structure):
    """deqsci_grad_entry"""
    _fields_ = [("grad", _ptr), ("numel", _i64)]


def _grad_table(grads, what):
    """-> (the deqsci_grad_entry table of the listed gradients, their device): fp32, dense, non-empty, on one HIP device"""
    dev = grads[0].device if grads else None
    table = (GradEntry * max(len(grads), 1))()
    for i, g in enumerate(grads):
        if not (isinstance(g, torch.Tensor) and g.is_cuda and g.dtype == torch.float32 and g.is_contiguous() and g.device == dev and g.numel() > 0):
            raise DeqsciHipError(f"{what}: gradient {i} must be a non-empty contiguous float32 tensor on {dev}; deqsci_amd has no CPU path")
        table[i].grad, table[i].numel = g.data_ptr(), g.numel()
    return table, dev


def grad_norm_launches(n_tensors):
    """The launches of grad_norm for n_tensors gradients: a chunk and a fold kernel per table of ADAM_MAX_TENSORS, one final kernel."""
    return 2 * -(-n_tensors // ADAM_MAX_TENSORS) + 1


def grad_norm_workspace(grads):
    """The caller-owned workspace of grad_norm for the listed gradients (float64 words; no initialisation needed)."""
    table, dev = _grad_table(grads, "grad_norm_workspace")
    return _partials(load().deqsci_grad_norm_workspace_bytes(ctypes.cast(table, _ptr), len(grads)), dev)


def grad_norm(grads, max_norm, stats=None, workspace=None):
    """L3: the global 2-norm of the listed gradients (any number; fp32, dense, on one device - views into a flat buffer will do) ->
    stats (3 + n,) float64 on their device: the norm, coef = fp32(min(1, max_norm / (norm + 1e-6))), the number of non-finite elements,
    then every tensor's own norm.  Deterministic (csrc/rows.hpp's order per tensor, then the list order: tests/clip_ref.py);
    grad_norm_launches(n) launches, no host synchronisation; stats / workspace: given by a caller that must not allocate."""
    n = len(grads)
    if n == 0:
        raise DeqsciHipError("grad_norm: no gradients (and so no device to put the norm on)")
    if not float(max_norm) >= 0.0:
        raise DeqsciHipError(f"grad_norm: max_norm must be >= 0, got {max_norm!r}")
    table, dev = _grad_table(grads, "grad_norm")
    if stats is None:
        stats = torch.empty((3 + n,), device=dev, dtype=torch.float64)
    elif stats.dtype != torch.float64 or stats.numel() != 3 + n or not stats.is_contiguous() or stats.device != dev:
        raise DeqsciHipError(f"grad_norm: stats must be 3 + {n} contiguous float64 values on {dev}")
    lib = load()
    workspace = _partials(lib.deqsci_grad_norm_workspace_bytes(ctypes.cast(table, _ptr), n), dev, workspace,
                          "grad_norm: workspace too small (grad_norm_workspace(grads))")
    with _dev(grads[0]):
        _check(lib.deqsci_grad_norm_f32(ctypes.cast(table, _ptr), n, float(max_norm), stats.data_ptr(), workspace.data_ptr(), _stream()), "grad_norm")
    return stats


def grad_scale_(grads, stats):
    """L3s: g *= stats[1] in place for the listed gradients (one fp32 rounding); nothing is written where stats[2] > 0 -> the launches."""
    n = len(grads)
    if n == 0:
        return 0
    table, dev = _grad_table(grads, "grad_scale_")
    if not (isinstance(stats, torch.Tensor) and stats.dtype == torch.float64 and stats.device == dev and stats.is_contiguous() and stats.numel() >= 3):
        raise DeqsciHipError(f"grad_scale_: stats must be at least 3 contiguous float64 values on {dev} (grad_norm's)")
    with _dev(grads[0]):
        _check(load().deqsci_grad_scale_f32(ctypes.cast(table, _ptr), n, stats.data_ptr(), _stream()), "grad_scale_")
    return -(-n // ADAM_MAX_TENSORS)


# ----------------------------------------------------------------------------- training batches out of raw video (csrc/synth.hip)
SYNTH_ROW_WORDS, SYNTH_MAX_ROWS, SYNTH_MAX_FRAMES = 10, 64, 64     # DEQSCI_SYNTH_ROW_WORDS, DEQSCI_SYNTH_MAX_ROWS, DEQSCI_SYNTH_MAX_FRAMES
SYNTH_FLIP_H, SYNTH_FLIP_V, SYNTH_TRANSPOSE = 1, 2, 4              # DEQSCI_SYNTH_FLIP_H, DEQSCI_SYNTH_FLIP_V, DEQSCI_SYNTH_TRANSPOSE


def synth_batch(pool, table, mask, H, W, B, gt=None, meas=None):
    """Y1: a training batch out of a pool of uint8 frames -> (gt (bsz,H,W,B), meas (bsz,H,W)), fp32 on the pool's device.  pool: a
    contiguous uint8 tensor on the device, every video a (T,Hv,Wv) block; table: bsz rows {video_offset, T, Hv, Wv, t0, dt, y0, x0, ds,
    flags} of int64 on the HOST (anything numpy turns into a (bsz, 10) int64 array); mask: fp32 (H,W,B), one for all samples, or
    (bsz,H,W,B).  The library checks every row against its video and the pool before it launches anything (a row that leaves them:
    DeqsciHipError, code -2).  No host synchronisation; gt / meas: given by a caller that must not allocate."""
    import numpy as np
    if not (isinstance(pool, torch.Tensor) and pool.is_cuda and pool.dtype == torch.uint8 and pool.is_contiguous()):
        raise DeqsciHipError("synth_batch: pool must be a contiguous uint8 tensor on a HIP device; deqsci_amd has no CPU path")
    rows = np.ascontiguousarray(np.asarray(table, dtype=np.int64))
    if rows.ndim != 2 or rows.shape[1] != SYNTH_ROW_WORDS:
        raise DeqsciHipError(f"synth_batch: the table must be (bsz, {SYNTH_ROW_WORDS}) integers, got {rows.shape}")
    bsz, H, W, B = rows.shape[0], int(H), int(W), int(B)
    if not (isinstance(mask, torch.Tensor) and mask.is_cuda and mask.dtype == torch.float32 and mask.is_contiguous() and mask.device == pool.device
            and tuple(mask.shape) in ((H, W, B), (bsz, H, W, B))):
        raise DeqsciHipError(f"synth_batch: mask must be a contiguous float32 tensor of shape ({H},{W},{B}) or ({bsz},{H},{W},{B}) on the pool's device")
    shapes = {"gt": (bsz, H, W, B), "meas": (bsz, H, W)}
    outs = {"gt": gt, "meas": meas}
    for name, t in outs.items():
        if t is None:
            outs[name] = torch.empty(shapes[name], device=pool.device, dtype=torch.float32)
        elif t.dtype != torch.float32 or tuple(t.shape) != shapes[name] or not t.is_contiguous() or t.device != pool.device:
            raise DeqsciHipError(f"synth_batch: {name} must be a contiguous float32 tensor of shape {shapes[name]} on the pool's device")
    stride = H * W * B if mask.dim() == 4 else 0
    with _dev(pool):
        _check(load().deqsci_synth_batch_u8(pool.data_ptr(), pool.numel(), rows.ctypes.data, bsz, mask.data_ptr(), stride, outs["gt"].data_ptr(),
                                            outs["meas"].data_ptr(), H, W, B, _stream()), "synth_batch")
    return outs["gt"], outs["meas"]


def rgb_to_gray(rgb, out=None):
    """Y0: (..., 3) uint8 RGB on the device -> (...) uint8, (77 R + 150 G + 29 B + 128) >> 8 in integers."""
    if not (isinstance(rgb, torch.Tensor) and rgb.is_cuda and rgb.dtype == torch.uint8 and rgb.is_contiguous() and rgb.dim() >= 1 and rgb.shape[-1] == 3):
        raise DeqsciHipError("rgb_to_gray: a contiguous uint8 tensor (..., 3) on a HIP device; deqsci_amd has no CPU path")
    if out is None:
        out = torch.empty(rgb.shape[:-1], device=rgb.device, dtype=torch.uint8)
    elif out.dtype != torch.uint8 or tuple(out.shape) != tuple(rgb.shape[:-1]) or not out.is_contiguous() or out.device != rgb.device:
        raise DeqsciHipError("rgb_to_gray: out must be a contiguous uint8 tensor of rgb's leading shape on rgb's device")
    with _dev(rgb):
        _check(load().deqsci_rgb_to_gray_u8(rgb.data_ptr(), out.data_ptr(), out.numel(), _stream()), "rgb_to_gray")
    return out


# ----------------------------------------------------------------------------- random source and sensor noise (csrc/noise.hip)
NOISE_MAX_ROWS = 64      # DEQSCI_NOISE_MAX_ROWS: samples per launch
_U64 = (1 << 64) - 1


def _seq_array(seq, what):
    """The per-sample sequence numbers as a contiguous uint64 HOST array (python ints of any size below 2^64, or an integer array)."""
    import numpy as np
    vals = [int(v) for v in np.asarray(seq, dtype=object).reshape(-1)]
    if any(v < 0 or v > _U64 for v in vals):
        raise DeqsciHipError(f"{what}: sequence numbers must lie in 0 .. 2^64 - 1")
    return np.asarray(vals, dtype=np.uint64)


def _noise_out(out, shape, dtype, device, what):
    if out is None:
        return torch.empty(shape, device=device, dtype=dtype)
    if not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == dtype and out.is_contiguous() and tuple(out.shape) == tuple(shape)):
        raise DeqsciHipError(f"{what}: out must be a contiguous {dtype} tensor of shape {tuple(shape)} on a HIP device")
    return out


def philox_words(seq, n, seed, device="cuda", out=None):
    """N0: the raw Philox4x32-10 words of the groups that serve n elements per sample -> (bsz, ceil(n / 4), 4) int32 holding the uint32 bit
    patterns (view them with .cpu().numpy().view(numpy.uint32)).  seq: bsz sequence numbers on the HOST; seed: the 64-bit key."""
    rows = _seq_array(seq, "philox_words")
    bsz, n = rows.size, int(n)
    out = _noise_out(out, (bsz, -(-n // 4), 4), torch.int32, device, "philox_words")
    with _dev(out):
        _check(load().deqsci_philox_words_u32(out.data_ptr(), rows.ctypes.data, bsz, n, int(seed) & _U64, _stream()), "philox_words")
    return out


def philox_normal(seq, n, seed, device="cuda", out=None):
    """N1: (bsz, n) fp32 standard normals; element e of the sample with sequence number seq[k] is a function of (seed, seq[k], e) alone."""
    rows = _seq_array(seq, "philox_normal")
    bsz, n = rows.size, int(n)
    out = _noise_out(out, (bsz, n), torch.float32, device, "philox_normal")
    with _dev(out):
        _check(load().deqsci_philox_normal_f32(out.data_ptr(), rows.ctypes.data, bsz, n, int(seed) & _U64, _stream()), "philox_normal")
    return out


def sensor_noise(y, seq, seed, sigma, gain, bits, full_scale, out=None):
    """N2: y (bsz, ...) -> y + sqrt(gain max(y, 0) + sigma^2) normal, quantised to `bits` bits over [0, full_scale] where bits > 0, in the
    order of operations include/deqsci_hip.h states.  out: None (a new tensor) or y itself (in place)."""
    rows = _seq_array(seq, "sensor_noise")
    bsz = rows.size
    _p(y, "y")
    if y.dim() < 1 or y.shape[0] != bsz:
        raise DeqsciHipError(f"sensor_noise: y {tuple(y.shape)} does not hold {bsz} samples")
    n = y.numel() // bsz if bsz else 1
    out = _noise_out(out, y.shape, torch.float32, y.device, "sensor_noise")
    if out.device != y.device:
        raise DeqsciHipError("sensor_noise: out must be on y's device")
    with _dev(y):
        _check(load().deqsci_sensor_noise_f32(y.data_ptr(), out.data_ptr(), rows.ctypes.data, bsz, n, int(seed) & _U64, float(sigma), float(gain),
                                              int(bits), float(full_scale), _stream()), "sensor_noise")
    return out


# ----------------------------------------------------------------------------- measurement helpers (bench.py)
class KernelTimer:
    """Per-launch kernel durations from the dispatch's own start/stop timestamps (the *_timed_f32 entry points record
    HIP events around the kernel on the stream it runs on).  All events are created up front (`capacity` launches) and
    destroyed by close(); launches beyond the capacity run untimed.  Read durations after synchronising the stream."""

    _plain_mix_gap = staticmethod(anderson_mix_gap)          # bound here: callers may monkey-patch the module names

    def __init__(self, capacity=0):
        self.events = []
        self.used = 0
        for _ in range(2 * capacity):
            h = _ptr()
            _check(load().deqsci_event_create(ctypes.byref(h)), "event_create")
            self.events.append(h)

    def _pair(self):
        if 2 * self.used + 1 >= len(self.events):
            return None
        e = self.events[2 * self.used], self.events[2 * self.used + 1]
        self.used += 1
        return e

    def reset(self):
        self.used = 0

    @property
    def full(self):
        return 2 * self.used + 1 >= len(self.events)

    def mix_gap(self, ws, beta, n, phi, y, phisum, x_out, z1, layout):
        ev = self._pair()
        if ev is None:
            return self._plain_mix_gap(ws, beta, n, phi, y, phisum, x_out, z1, layout)
        bsz, H, W, B = _dims(layout, z1.shape)
        with _dev(ws.F):
            _check(load().deqsci_anderson_mix_gap_timed_f32(
                _p(ws.F), _p(ws.G), _p(ws.alpha), float(beta), n, ws.m, _p(phi, "Phi"), _p(y, "y"), _p(phisum, "Phi_sum"),
                _p(x_out, "x_out"), _p(z1, "z1"), bsz, H, W, B, layout, _phi_shared(phi, bsz), _stream(), ev[0], ev[1]),
                "anderson_mix_gap_timed")

    def pair(self):
        """The next unused (start, stop) pair, or None when the capacity is used up (for CONV64_EVENT_HOOK)."""
        return self._pair()

    def durations_ms(self):
        out = []
        ms = _f32()
        for i in range(self.used):
            _check(load().deqsci_event_elapsed_ms(self.events[2 * i], self.events[2 * i + 1], ctypes.byref(ms)), "event_elapsed_ms")
            out.append(ms.value)
        return out

    def close(self):
        for e in self.events:
            load().deqsci_event_destroy(e)
        self.events, self.used = [], 0
