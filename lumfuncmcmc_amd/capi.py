"""ctypes binding of liblfmcmc.so (include/lfmcmc.h).

There is no CPU fallback: if the shared object is missing or does not load, importing
callers get a RuntimeError that says so.  Build it with `python -m lumfuncmcmc_amd.build`
(or `__graft_entry__.build()`).
"""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "liblfmcmc.so")

LF_ABI_VERSION = 3
LF_MAX_FIELDS = 8
LF_FREE, LF_FIXCOMP, LF_ZEVOL = 0, 1, 2
VARIANTS = {"free": LF_FREE, "fixcomp": LF_FIXCOMP, "zevol": LF_ZEVOL}
LF_OK = 0
LF_ERR_ARG = -1
LF_Q_LINEAR, LF_Q_MEDIAN = 0, 1
LF_INT_NUMBER, LF_INT_LUMDENS = 0, 1
LIM_ORDER = ("Lstar", "phistar", "sch_al", "Flim", "alpha")

MPC_CM = 3.086e24                                  # lumfuncmcmc.py:70

_c_double_p = ctypes.POINTER(ctypes.c_double)
_c_int64_p = ctypes.POINTER(ctypes.c_int64)


class LfDesc(ctypes.Structure):
    _fields_ = [
        ("variant", ctypes.c_int32), ("fix_sch_al", ctypes.c_int32),
        ("nf", ctypes.c_int32), ("S", ctypes.c_int32), ("N", ctypes.c_int64),
        ("field_ind", _c_int64_p), ("lum", _c_double_p), ("logf", _c_double_p),
        ("z", _c_double_p), ("om_arr", _c_double_p), ("omega0", _c_double_p),
        ("logL", _c_double_p), ("zarr", _c_double_p), ("volume_part", _c_double_p),
        ("dl_zarr", _c_double_p), ("integ_part", _c_double_p), ("flim0", _c_double_p),
        ("alpha0", ctypes.c_double), ("sch_al0", ctypes.c_double), ("fcmin", ctypes.c_double),
        ("lims", (ctypes.c_double * 2) * 5), ("pivots", ctypes.c_double * 3),
        ("device", ctypes.c_int32), ("max_batch", ctypes.c_int32),
    ]


EXPORTS = ("lf_abi_version", "lf_create", "lf_destroy", "lf_ndim", "lf_lnprob_batch",
           "lf_lnprob_batch_device", "lf_lnprob_batch_device_n", "lf_lnprob_pieces", "lf_set_profiling", "lf_kernel_times",
           "lf_set_option", "lf_last_error", "lf_sampler_create", "lf_sampler_destroy", "lf_sampler_start",
           "lf_sampler_run", "lf_sampler_read", "lf_sampler_steps", "lf_sampler_half_eval",
           "lf_sampler_half_accept", "lf_compress_keys", "lf_compress_grid", "lf_grid_bins", "lf_deal_table", "lf_deal_finishers", "lf_form_counts", "lf_last_launch",
           "lf_free_block_uploads", "lf_veff",
           "lf_lumfunc_quantiles", "lf_lumfunc_quantiles_ms", "lf_ptsampler_create", "lf_ptsampler_destroy",
           "lf_ptsampler_start", "lf_ptsampler_run", "lf_ptsampler_read", "lf_ptsampler_steps", "lf_mock_create",
           "lf_mock_destroy", "lf_mock_counts", "lf_mock_draw", "lf_mock_hist", "lf_mock_last_error", "lf_chain_diag",
           "lf_sampler_diag", "lf_ptsampler_diag", "lf_chain_window", "lf_diag_last", "lf_lnprob_grad_batch",
           "lf_lnprob_grad_batch_device", "lf_lumfunc_integral_quantiles", "lf_lumfunc_integral_quantiles_ms", "lf_veff_draws", "lf_veff_draws_ms",
           "lf_veff_draws_chunk", "lf_veff_draws_zmax", "lf_set_lum_err", "lf_lnprob_err_batch", "lf_lnprob_err_batch_device", "lf_gauss_hermite",
           "lf_deconv_info", "lf_deconv_wide_info", "lf_lnprob_err_grad_batch", "lf_lnprob_err_grad_batch_device", "lf_sampler_set_likelihood",
           "lf_ptsampler_set_likelihood", "lf_lum_posterior", "lf_lum_posterior_info",
           "lf_veff_true", "lf_veff_true_info", "lf_veff_true_ms",
           "lf_mock_set_error_model", "lf_mock_draw_err", "lf_mock_hist_err",
           "lf_set_cut_error_model", "lf_cut_term_batch", "lf_cut_info", "lf_cut_term_grad_batch",
           "lf_mock_set_cut_band", "lf_mock_draw_cut", "lf_mock_hist_cut",
           "lf_veff_true_cut", "lf_veff_true_cut_info", "lf_veff_true_cut_ms", "lf_cut_volume",
           "lf_veff_slices", "lf_veff_slices_ms")
# the mocks binned in (z, logL).  Kept apart from EXPORTS: tests/test_capi_cpu.py compares that tuple
# with a scan of the header that reads names made of letters and underscores only.
EXPORTS_HIST2 = ("lf_mock_hist2", "lf_mock_hist2_err", "lf_mock_hist2_cut")

_lib = None


def load():
    """dlopen liblfmcmc.so and declare the prototypes.  Raises RuntimeError if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "liblfmcmc.so not found at %s: the HIP library has not been built "
            "(run `python -m lumfuncmcmc_amd.build`). There is no CPU fallback." % LIB_PATH)
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64.so.7 / libhsa-runtime64,
    # and a second runtime initialised in the same process sees no GPU.  Importing torch first
    # makes the dynamic loader resolve this library's libamdhip64.so.7 to torch's copy, so device
    # pointers and streams can be shared with torch (and with RCCL through torch.distributed).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    try:
        lib = ctypes.CDLL(LIB_PATH)
    except OSError as e:
        raise RuntimeError("liblfmcmc.so failed to load (%s). There is no CPU fallback." % e)
    # a library built from older sources lacks entries the binding declares (the ABI version only moves when existing
    # entries change): say so here rather than at the first call
    missing = [n for n in EXPORTS + EXPORTS_HIST2 if not hasattr(lib, n)]
    if missing:
        raise RuntimeError("liblfmcmc.so at %s lacks %s: rebuild the library (python -m lumfuncmcmc_amd.build --force)"
                           % (LIB_PATH, ", ".join(missing)))
    lib.lf_abi_version.restype = ctypes.c_int
    lib.lf_abi_version.argtypes = []
    lib.lf_create.restype = ctypes.c_void_p
    lib.lf_create.argtypes = [ctypes.POINTER(LfDesc)]
    lib.lf_destroy.restype = None
    lib.lf_destroy.argtypes = [ctypes.c_void_p]
    lib.lf_ndim.restype = ctypes.c_int
    lib.lf_ndim.argtypes = [ctypes.c_void_p]
    lib.lf_lnprob_batch.restype = ctypes.c_int
    lib.lf_lnprob_batch.argtypes = [ctypes.c_void_p, _c_double_p, ctypes.c_int, _c_double_p]
    lib.lf_lnprob_batch_device.restype = ctypes.c_int
    lib.lf_lnprob_batch_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                           ctypes.c_void_p, ctypes.c_void_p]
    lib.lf_lnprob_batch_device_n.restype = ctypes.c_int
    lib.lf_lnprob_batch_device_n.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                             ctypes.c_void_p, ctypes.c_void_p]
    lib.lf_lnprob_grad_batch.restype = ctypes.c_int
    lib.lf_lnprob_grad_batch.argtypes = [ctypes.c_void_p, _c_double_p, ctypes.c_int, _c_double_p, _c_double_p]
    lib.lf_lnprob_grad_batch_device.restype = ctypes.c_int
    lib.lf_lnprob_grad_batch_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                                ctypes.c_void_p]
    lib.lf_set_lum_err.restype = ctypes.c_int
    lib.lf_set_lum_err.argtypes = [ctypes.c_void_p, _c_double_p, ctypes.c_int, _c_double_p, _c_double_p, ctypes.c_double]
    lib.lf_lnprob_err_batch.restype = ctypes.c_int
    lib.lf_lnprob_err_batch.argtypes = [ctypes.c_void_p, _c_double_p, ctypes.c_int, _c_double_p]
    lib.lf_lnprob_err_batch_device.restype = ctypes.c_int
    lib.lf_lnprob_err_batch_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lib.lf_set_cut_error_model.restype = ctypes.c_int
    lib.lf_set_cut_error_model.argtypes = [ctypes.c_void_p, _c_double_p, ctypes.c_int, _c_double_p]
    lib.lf_cut_term_batch.restype = ctypes.c_int
    lib.lf_cut_term_batch.argtypes = [ctypes.c_void_p, _c_double_p, ctypes.c_int, _c_double_p]
    lib.lf_cut_term_grad_batch.restype = ctypes.c_int
    lib.lf_cut_term_grad_batch.argtypes = [ctypes.c_void_p, _c_double_p, ctypes.c_int, _c_double_p, _c_double_p]
    lib.lf_cut_info.restype = ctypes.c_int
    lib.lf_cut_info.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32), _c_double_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                                ctypes.POINTER(ctypes.c_int)]
    lib.lf_gauss_hermite.restype = ctypes.c_int
    lib.lf_gauss_hermite.argtypes = [ctypes.c_int, _c_double_p, _c_double_p]
    lib.lf_lnprob_err_grad_batch.restype = ctypes.c_int
    lib.lf_lnprob_err_grad_batch.argtypes = [ctypes.c_void_p, _c_double_p, ctypes.c_int, _c_double_p, _c_double_p]
    lib.lf_lnprob_err_grad_batch_device.restype = ctypes.c_int
    lib.lf_lnprob_err_grad_batch_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                                    ctypes.c_void_p]
    lib.lf_lum_posterior.restype = ctypes.c_int
    lib.lf_lum_posterior.argtypes = [ctypes.c_void_p, _c_double_p, ctypes.c_int, _c_double_p, _c_double_p, ctypes.POINTER(ctypes.c_int)]
    lib.lf_lum_posterior_info.restype = ctypes.c_int
    lib.lf_lum_posterior_info.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    lib.lf_veff_true.restype = ctypes.c_int
    lib.lf_veff_true.argtypes = [ctypes.c_void_p, _c_double_p, ctypes.c_int, _c_double_p, ctypes.c_int, ctypes.c_double, ctypes.c_double,
                                 ctypes.c_int, _c_double_p, ctypes.c_int, _c_double_p, _c_double_p, ctypes.POINTER(ctypes.c_int)]
    lib.lf_veff_true_cut.restype = ctypes.c_int
    lib.lf_veff_true_cut.argtypes = (lib.lf_veff_true.argtypes[:7] + [ctypes.c_double] + lib.lf_veff_true.argtypes[7:])
    lib.lf_veff_true_cut_info.restype = ctypes.c_int
    lib.lf_veff_true_cut_info.argtypes = [ctypes.c_void_p, _c_int64_p, _c_int64_p, _c_int64_p]
    lib.lf_veff_true_cut_ms.restype = ctypes.c_int
    lib.lf_veff_true_cut_ms.argtypes = [ctypes.c_void_p, _c_double_p]
    lib.lf_cut_volume.restype = ctypes.c_int
    lib.lf_cut_volume.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32), _c_double_p, ctypes.c_int64, _c_double_p]
    lib.lf_veff_true_info.restype = ctypes.c_int
    lib.lf_veff_true_info.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    lib.lf_veff_true_ms.restype = ctypes.c_int
    lib.lf_veff_true_ms.argtypes = [_c_double_p]
    lib.lf_deconv_wide_info.restype = ctypes.c_int
    lib.lf_deconv_wide_info.argtypes = [_c_double_p, ctypes.POINTER(ctypes.c_int32), ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                                        _c_double_p, ctypes.POINTER(ctypes.c_int), _c_double_p, ctypes.c_int, _c_double_p, _c_double_p]
    lib.lf_deconv_info.restype = ctypes.c_int
    lib.lf_deconv_info.argtypes = [ctypes.POINTER(ctypes.c_int32), _c_double_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                                   ctypes.POINTER(ctypes.c_int)]
    lib.lf_lnprob_pieces.restype = ctypes.c_int
    lib.lf_lnprob_pieces.argtypes = [ctypes.c_void_p, _c_double_p, ctypes.c_int, _c_double_p, _c_double_p]
    lib.lf_set_profiling.restype = ctypes.c_int
    lib.lf_set_profiling.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.lf_kernel_times.restype = ctypes.c_int
    lib.lf_kernel_times.argtypes = [ctypes.c_void_p, _c_double_p, _c_int64_p]
    lib.lf_set_option.restype = ctypes.c_int
    lib.lf_set_option.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int64]
    lib.lf_form_counts.restype = ctypes.c_int
    lib.lf_form_counts.argtypes = [ctypes.c_void_p, _c_int64_p]
    lib.lf_last_launch.restype = ctypes.c_int
    lib.lf_last_launch.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32)]
    lib.lf_free_block_uploads.restype = ctypes.c_int
    lib.lf_free_block_uploads.argtypes = [ctypes.c_void_p, _c_int64_p]
    lib.lf_veff.restype = ctypes.c_int
    lib.lf_veff.argtypes = [ctypes.c_int, ctypes.c_int64, _c_double_p, _c_double_p, _c_double_p, ctypes.c_double, ctypes.c_double,
                            ctypes.c_double, ctypes.c_double, ctypes.POINTER(ctypes.c_int32), ctypes.c_int32, ctypes.c_int32,
                            _c_int64_p, ctypes.c_uint64, _c_double_p, _c_double_p]
    lib.lf_veff_slices.restype = ctypes.c_int
    lib.lf_veff_slices.argtypes = [ctypes.c_int, ctypes.c_int64, _c_double_p, _c_double_p, _c_double_p, ctypes.c_double, ctypes.c_double,
                                   ctypes.c_double, ctypes.POINTER(ctypes.c_int32), ctypes.c_int32, ctypes.POINTER(ctypes.c_int32),
                                   ctypes.c_int32, ctypes.c_int32, _c_int64_p, ctypes.c_uint64, _c_double_p, _c_double_p, _c_int64_p]
    lib.lf_veff_slices_ms.restype = ctypes.c_double
    lib.lf_veff_slices_ms.argtypes = []
    lib.lf_lumfunc_quantiles.restype = ctypes.c_int
    lib.lf_lumfunc_quantiles.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int32, _c_double_p, ctypes.c_int64, _c_double_p,
                                         _c_double_p, ctypes.c_int32, _c_double_p, ctypes.c_int32, _c_double_p, _c_double_p]
    lib.lf_lumfunc_quantiles_ms.restype = ctypes.c_int
    lib.lf_lumfunc_quantiles_ms.argtypes = [_c_double_p]
    lib.lf_lumfunc_integral_quantiles.restype = ctypes.c_int
    lib.lf_lumfunc_integral_quantiles.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int32, _c_double_p,
                                                  ctypes.c_int64, _c_double_p, _c_double_p, ctypes.c_int32, _c_double_p,
                                                  ctypes.c_int32, _c_double_p, _c_double_p]
    lib.lf_lumfunc_integral_quantiles_ms.restype = ctypes.c_int
    lib.lf_lumfunc_integral_quantiles_ms.argtypes = [_c_double_p]
    lib.lf_veff_draws.restype = ctypes.c_int
    lib.lf_veff_draws.argtypes = [ctypes.c_int, ctypes.c_int64, _c_double_p, ctypes.POINTER(ctypes.c_int32), _c_double_p, ctypes.c_double,
                                  ctypes.c_double, ctypes.c_double, ctypes.POINTER(ctypes.c_int32), ctypes.c_int32, ctypes.c_int32,
                                  ctypes.c_int32, _c_double_p, ctypes.c_int32, _c_double_p, ctypes.c_int32, _c_double_p, _c_double_p]
    lib.lf_veff_draws_zmax.restype = ctypes.c_int
    lib.lf_veff_draws_zmax.argtypes = [ctypes.c_int, ctypes.c_int64, _c_double_p, ctypes.POINTER(ctypes.c_int32), _c_double_p, ctypes.c_double,
                                       ctypes.c_double, ctypes.POINTER(ctypes.c_int32), ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                       _c_double_p, _c_double_p, _c_double_p, _c_double_p, _c_double_p, ctypes.c_int64, ctypes.c_int32,
                                       _c_double_p, ctypes.c_int32, _c_double_p, _c_double_p]
    lib.lf_veff_draws_ms.restype = ctypes.c_int
    lib.lf_veff_draws_ms.argtypes = [_c_double_p]
    lib.lf_veff_draws_chunk.restype = ctypes.c_int
    lib.lf_veff_draws_chunk.argtypes = []
    lib.lf_last_error.restype = ctypes.c_char_p
    lib.lf_last_error.argtypes = [ctypes.c_void_p]
    lib.lf_sampler_create.restype = ctypes.c_void_p
    lib.lf_sampler_create.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_uint64, ctypes.c_int64]
    lib.lf_sampler_destroy.restype = None
    lib.lf_sampler_destroy.argtypes = [ctypes.c_void_p]
    lib.lf_sampler_start.restype = ctypes.c_int
    lib.lf_sampler_start.argtypes = [ctypes.c_void_p, _c_double_p, _c_double_p]
    lib.lf_sampler_run.restype = ctypes.c_int
    lib.lf_sampler_run.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    lib.lf_sampler_read.restype = ctypes.c_int
    lib.lf_sampler_read.argtypes = [ctypes.c_void_p, _c_double_p, _c_double_p, _c_int64_p, _c_double_p, _c_double_p]
    lib.lf_sampler_steps.restype = ctypes.c_int64
    lib.lf_sampler_steps.argtypes = [ctypes.c_void_p]
    lib.lf_sampler_half_eval.restype = ctypes.c_int
    lib.lf_sampler_half_eval.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lib.lf_sampler_half_accept.restype = ctypes.c_int
    lib.lf_sampler_half_accept.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lib.lf_sampler_set_likelihood.restype = ctypes.c_int
    lib.lf_sampler_set_likelihood.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.lf_ptsampler_set_likelihood.restype = ctypes.c_int
    lib.lf_ptsampler_set_likelihood.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.lf_ptsampler_create.restype = ctypes.c_void_p
    lib.lf_ptsampler_create.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, _c_double_p, ctypes.c_double, ctypes.c_uint64,
                                        ctypes.c_int64]
    lib.lf_ptsampler_destroy.restype = None
    lib.lf_ptsampler_destroy.argtypes = [ctypes.c_void_p]
    lib.lf_ptsampler_start.restype = ctypes.c_int
    lib.lf_ptsampler_start.argtypes = [ctypes.c_void_p, _c_double_p, _c_double_p]
    lib.lf_ptsampler_run.restype = ctypes.c_int
    lib.lf_ptsampler_run.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    lib.lf_ptsampler_read.restype = ctypes.c_int
    lib.lf_ptsampler_read.argtypes = [ctypes.c_void_p, _c_double_p, _c_double_p, _c_double_p, _c_int64_p, _c_int64_p, _c_double_p,
                                      _c_double_p]
    lib.lf_ptsampler_steps.restype = ctypes.c_int64
    lib.lf_ptsampler_steps.argtypes = [ctypes.c_void_p]
    lib.lf_mock_create.restype = ctypes.c_void_p
    lib.lf_mock_create.argtypes = [ctypes.POINTER(LfDesc)]
    lib.lf_mock_destroy.restype = None
    lib.lf_mock_destroy.argtypes = [ctypes.c_void_p]
    lib.lf_mock_counts.restype = ctypes.c_int
    lib.lf_mock_counts.argtypes = [ctypes.c_void_p, _c_double_p, ctypes.c_int32, _c_int64_p, ctypes.c_uint64, _c_double_p, _c_int64_p]
    lib.lf_mock_draw.restype = ctypes.c_int
    lib.lf_mock_draw.argtypes = [ctypes.c_void_p, _c_double_p, ctypes.c_int32, _c_int64_p, ctypes.c_uint64, _c_int64_p, _c_double_p,
                                 _c_double_p, ctypes.POINTER(ctypes.c_int32)]
    lib.lf_mock_hist.restype = ctypes.c_int
    lib.lf_mock_hist.argtypes = [ctypes.c_void_p, _c_double_p, ctypes.c_int32, _c_int64_p, ctypes.c_uint64, ctypes.c_int32, _c_double_p,
                                 _c_int64_p]
    lib.lf_mock_set_error_model.restype = ctypes.c_int
    lib.lf_mock_set_error_model.argtypes = [ctypes.c_void_p, ctypes.c_int32, _c_double_p, _c_double_p, _c_double_p]
    lib.lf_mock_draw_err.restype = ctypes.c_int
    lib.lf_mock_draw_err.argtypes = [ctypes.c_void_p, _c_double_p, ctypes.c_int32, _c_int64_p, ctypes.c_uint64, _c_int64_p, _c_double_p,
                                     _c_double_p, _c_double_p, _c_double_p, ctypes.POINTER(ctypes.c_int32)]
    lib.lf_mock_hist_err.restype = ctypes.c_int
    lib.lf_mock_hist_err.argtypes = lib.lf_mock_hist.argtypes
    lib.lf_mock_set_cut_band.restype = ctypes.c_int
    lib.lf_mock_set_cut_band.argtypes = [ctypes.c_void_p, _c_double_p, _c_double_p]
    lib.lf_mock_draw_cut.restype = ctypes.c_int
    lib.lf_mock_draw_cut.argtypes = [ctypes.c_void_p, _c_double_p, ctypes.c_int32, _c_int64_p, ctypes.c_uint64, ctypes.c_int64, _c_double_p,
                                     _c_double_p, _c_double_p, _c_double_p, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32),
                                     _c_int64_p, _c_double_p, _c_int64_p]
    lib.lf_mock_hist_cut.restype = ctypes.c_int
    lib.lf_mock_hist_cut.argtypes = lib.lf_mock_hist.argtypes + [_c_int64_p]
    lib.lf_mock_hist2.restype = ctypes.c_int
    lib.lf_mock_hist2.argtypes = [ctypes.c_void_p, _c_double_p, ctypes.c_int32, _c_int64_p, ctypes.c_uint64, _c_int64_p, ctypes.c_int32,
                                  _c_double_p, ctypes.c_int32, _c_double_p, _c_int64_p]
    lib.lf_mock_hist2_err.restype = ctypes.c_int
    lib.lf_mock_hist2_err.argtypes = lib.lf_mock_hist2.argtypes
    lib.lf_mock_hist2_cut.restype = ctypes.c_int
    lib.lf_mock_hist2_cut.argtypes = [ctypes.c_void_p, _c_double_p, ctypes.c_int32, _c_int64_p, ctypes.c_uint64, ctypes.c_int32,
                                      _c_double_p, ctypes.c_int32, _c_double_p, _c_int64_p, _c_int64_p]
    lib.lf_mock_last_error.restype = ctypes.c_char_p
    lib.lf_mock_last_error.argtypes = [ctypes.c_void_p]
    lib.lf_compress_keys.restype = ctypes.c_int64
    lib.lf_compress_keys.argtypes = [ctypes.c_int, _c_double_p, _c_double_p, _c_double_p, ctypes.c_int64,
                                     _c_double_p, _c_double_p, ctypes.c_int64, _c_double_p]
    lib.lf_chain_diag.restype = ctypes.c_int
    lib.lf_chain_diag.argtypes = [ctypes.c_int, _c_double_p, _c_double_p, ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_int64,
                                  ctypes.c_int64, ctypes.c_double, _c_double_p, _c_int64_p, _c_double_p, _c_double_p, _c_double_p,
                                  ctypes.c_int64]
    lib.lf_sampler_diag.restype = ctypes.c_int
    lib.lf_sampler_diag.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_double, ctypes.c_int, _c_double_p, _c_int64_p, _c_double_p,
                                    _c_double_p]
    lib.lf_ptsampler_diag.restype = ctypes.c_int
    lib.lf_ptsampler_diag.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double, ctypes.c_int, _c_double_p,
                                      _c_int64_p, _c_double_p, _c_double_p]
    lib.lf_chain_window.restype = ctypes.c_int
    lib.lf_chain_window.argtypes = [_c_double_p, ctypes.c_int64, ctypes.c_double, ctypes.c_int64, _c_double_p, _c_int64_p]
    lib.lf_diag_last.restype = ctypes.c_int
    lib.lf_diag_last.argtypes = [_c_double_p, _c_int64_p]
    v = lib.lf_abi_version()
    if v != LF_ABI_VERSION:
        raise RuntimeError("liblfmcmc.so ABI %d != binding ABI %d: rebuild the library" % (v, LF_ABI_VERSION))
    _lib = lib
    return lib


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def compress_keys(kind, params, key, weight=None):
    """Host-only helper behind the "compress" option (csrc/lf_compress.h): replace the coordinates `key`
    (weights `weight`, default 1) by weighted pseudo-sources.  kind 0 = FREE (params = |a/(1-a)|, alpha_lo,
    alpha_hi, flim_lo, flim_hi), kind 1 = ZEVOL (params = L_lo, L_hi, z1, z2, z3).
    Returns (node, weight, bound).  Touches no GPU."""
    lib = load()
    params, key = _f64(params), _f64(key)
    wt = _f64(weight) if weight is not None else None
    cap = key.size + 64
    node, w = np.empty(cap), np.empty(cap)
    bound = np.zeros(1)
    n = lib.lf_compress_keys(int(kind), _ptr(params), _ptr(key), _ptr(wt), key.size, _ptr(node), _ptr(w), cap, _ptr(bound))
    if n < 0:
        raise RuntimeError("lf_compress_keys failed (%d): the error bound cannot be met" % n)
    return node[:n].copy(), w[:n].copy(), float(bound[0])


def compress_grid(params, L, wL, ck, Dk):
    """Host-only helper behind the compressed FREE grid (csrc/lf_compress.h: compress_grid).  Returns a dict with
    u (nb, 16), row0, nrows, off, omega (flat, per bin [row][node]) and bound.  Touches no GPU."""
    lib = load()
    params, L, wL, ck, Dk = (_f64(a) for a in (params, L, wL, ck, Dk))
    S = L.size
    capb, capo = 4096, 4096 * 16 * 64
    u = np.empty(capb * 16)
    row0, nrows, off = (np.empty(capb, dtype=np.int32) for _ in range(3))
    omega = np.empty(capo)
    bound = np.zeros(1)
    ip = ctypes.POINTER(ctypes.c_int32)
    lib.lf_compress_grid.restype = ctypes.c_int64
    lib.lf_compress_grid.argtypes = [_c_double_p, ctypes.c_int] + [_c_double_p] * 5 + [ip, ip, ip, _c_double_p,
                                                                                       ctypes.c_int64, ctypes.c_int64, _c_double_p]
    nb = lib.lf_compress_grid(_ptr(params), S, _ptr(L), _ptr(wL), _ptr(ck), _ptr(Dk), _ptr(u), row0.ctypes.data_as(ip),
                              nrows.ctypes.data_as(ip), off.ctypes.data_as(ip), _ptr(omega), capb, capo, _ptr(bound))
    if nb < 0:
        raise RuntimeError("lf_compress_grid failed (%d)" % nb)
    nom = int(off[nb - 1] + nrows[nb - 1] * 16)
    return {"u": u[:nb * 16].reshape(nb, 16).copy(), "row0": row0[:nb].copy(), "nrows": nrows[:nb].copy(),
            "off": off[:nb].copy(), "omega": omega[:nom].copy(), "bound": float(bound[0])}


def deal_table(n_cell_chunks, n_bins, grid_part=0, grid_parts=0):
    """Host-only helper behind lf_free's deal of its cell chunks and flux bins to its 32 virtual workgroups (csrc/lf_hostprep.h:
    make_deal).  Returns (cells, bins): two lists of 32 lists - the chunk / bin numbers each rank
    takes, in the order it takes them.  Touches no GPU."""
    lib = load()
    lib.lf_deal_table.restype = ctypes.c_int
    lib.lf_deal_table.argtypes = [ctypes.c_int] * 4 + [ctypes.POINTER(ctypes.c_int32), ctypes.c_int64]
    n = lib.lf_deal_table(int(n_cell_chunks), int(n_bins), int(grid_part), int(grid_parts), None, 0)
    if n < 0:
        raise ValueError("lf_deal_table: bad arguments")
    t = np.empty(n, dtype=np.int32)
    assert lib.lf_deal_table(int(n_cell_chunks), int(n_bins), int(grid_part), int(grid_parts), t.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), n) == n
    VF = (n - n_cell_chunks - n_bins) // 2 - 1
    lst = t[2 * (VF + 1):]
    cells = [lst[t[v]:t[v + 1]].tolist() for v in range(VF)]
    bins = [lst[n_cell_chunks + t[VF + 1 + v]:n_cell_chunks + t[VF + 2 + v]].tolist() for v in range(VF)]
    return cells, bins


def deal_finishers(n_cell_chunks, n_bins, grid_part=0, grid_parts=0):
    """Host-only: the physical rank that finishes a tile of lf_free's polling hand-over, for tiles served by 8, 16, 24 and 32
    workgroups (csrc/lf_hostprep.h: deal_finishers) - the rank the deal of deal_table() loads most.
    Touches no GPU."""
    lib = load()
    lib.lf_deal_finishers.restype = ctypes.c_int
    lib.lf_deal_finishers.argtypes = [ctypes.c_int] * 4 + [ctypes.POINTER(ctypes.c_int32)]
    r = (ctypes.c_int32 * 4)()
    if lib.lf_deal_finishers(int(n_cell_chunks), int(n_bins), int(grid_part), int(grid_parts), r) != 0:
        raise ValueError("lf_deal_finishers: bad arguments")
    return [int(v) for v in r]


def grid_bins(params, L, wL, ck, Dk):
    """Host-only helper behind piece B over flux bins (csrc/lf_gridbound.h: build_gridq; the default of FREE contexts with
    a separable grid).  params = |a/(1-a)|, alpha_lo, alpha_hi, flim_lo, flim_hi.  Returns a dict with edges (nb, 2), rec
    (nb, 64, 4) = {x_n, 10^(x_n + 17), L of row row0 + n, 10^(that - 42)}, rows (nb, 4) = {row0, nrows, offset, 0}, omega
    (flat, per bin [row][64]) and margin = ln(proven bound / allowance) <= 0.  Touches no GPU."""
    lib = load()
    params, L, wL, ck, Dk = (_f64(a) for a in (params, L, wL, ck, Dk))
    S = L.size
    capb, capo = 1024, 1024 * 64 * 64
    edges, rec = np.empty(capb * 2), np.empty(capb * 64 * 4)
    rows = np.empty(capb * 4, dtype=np.int32)
    omega = np.empty(capo)
    margin = np.zeros(1)
    ip = ctypes.POINTER(ctypes.c_int32)
    lib.lf_grid_bins.restype = ctypes.c_int64
    lib.lf_grid_bins.argtypes = [_c_double_p, ctypes.c_int] + [_c_double_p] * 6 + [ip, _c_double_p, ctypes.c_int64, ctypes.c_int64,
                                                                                   _c_double_p]
    nb = lib.lf_grid_bins(_ptr(params), S, _ptr(L), _ptr(wL), _ptr(ck), _ptr(Dk), _ptr(edges), _ptr(rec), rows.ctypes.data_as(ip),
                          _ptr(omega), capb, capo, _ptr(margin))
    if nb < 0:
        raise RuntimeError("lf_grid_bins failed (%d): no proven set of bins for this box" % nb)
    rows = rows[:nb * 4].reshape(nb, 4).copy()
    nom = int(rows[-1, 2] + rows[-1, 1] * 64)
    return {"edges": edges[:nb * 2].reshape(nb, 2).copy(), "rec": rec[:nb * 256].reshape(nb, 64, 4).copy(), "rows": rows,
            "omega": omega[:nom].copy(), "margin": float(margin[0])}


def veff_device(flux, flim, vol, pref0, alpha, fcmin, bin_of=None, nbin=0, nboot=0, boot_idx=None, seed=0, device=0):
    """lf_veff (include/lfmcmc.h): 1/Veff weights, and optionally their binned sums over the catalogue and over nboot
    bootstrap resamples, on the GPU.  vol: scalar or per-source array.  Returns (phi[n], sums[(nboot + 1), nbin] or None)."""
    lib = load()
    flux, flim = _f64(flux), _f64(flim)
    n = flux.size
    volarr = None if np.ndim(vol) == 0 else _f64(vol)
    phi = np.empty(n)
    sums = np.zeros((nboot + 1, nbin)) if nbin > 0 else None
    b32 = None if bin_of is None else np.ascontiguousarray(bin_of, dtype=np.int32)
    bidx = None if boot_idx is None else np.ascontiguousarray(boot_idx, dtype=np.int64)
    if bidx is not None and bidx.shape != (nboot, n):
        raise ValueError("boot_idx must be (nboot, n)")
    rc = lib.lf_veff(int(device), n, _ptr(flux), _ptr(flim), _ptr(volarr), float(vol) if volarr is None else 0.0, float(pref0),
                     float(alpha), float(fcmin) if fcmin else 0.0,
                     None if b32 is None else b32.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), int(nbin), int(nboot),
                     None if bidx is None else bidx.ctypes.data_as(_c_int64_p), ctypes.c_uint64(int(seed)), _ptr(phi),
                     None if sums is None else _ptr(sums))
    if rc != LF_OK:
        raise LFError("lf_veff failed (%d)" % rc)
    return phi, sums


def veff_slices(flux, flim, vol, pref0, alpha, fcmin, slice_of, nslice, bin_of, nbin, nboot=0, boot_idx=None, seed=0, device=0):
    """lf_veff_slices (include/lfmcmc.h): the 1/Veff weights with a volume per source, their binned sums per redshift slice
    over the catalogue and over nboot bootstrap resamples of each slice, and the catalogue's counts.  slice_of outside
    [0, nslice): no slice; bin_of outside [0, nbin): no bin; boot_idx (nboot, m): the draws as source numbers within the slice,
    for the m sources with a slice in slice-sorted order.  Returns (phi[n], sums[nboot + 1, nslice, nbin], counts[nslice, nbin]).
    The arguments are checked by the library before the device is touched: LFError."""
    lib = load()
    flux, flim, vol = _f64(flux), _f64(flim), _f64(vol)
    n = flux.size
    ip = ctypes.POINTER(ctypes.c_int32)
    s32 = np.ascontiguousarray(slice_of, dtype=np.int32)
    b32 = np.ascontiguousarray(bin_of, dtype=np.int32)
    if not (flim.size == vol.size == s32.size == b32.size == n):
        raise ValueError("flux, flim, vol, slice_of and bin_of must have one length")
    bidx = None if boot_idx is None else np.ascontiguousarray(boot_idx, dtype=np.int64)
    m = int(((s32 >= 0) & (s32 < nslice)).sum())
    if bidx is not None and bidx.shape != (nboot, m):
        raise ValueError("boot_idx must be (nboot, sources with a slice)")
    phi = np.empty(n)
    sums = np.zeros((max(int(nboot), 0) + 1, max(int(nslice), 0), max(int(nbin), 0)))
    counts = np.zeros((max(int(nslice), 0), max(int(nbin), 0)), dtype=np.int64)
    rc = lib.lf_veff_slices(int(device), n, _ptr(flux), _ptr(flim), _ptr(vol), float(pref0), float(alpha), float(fcmin) if fcmin else 0.0,
                            s32.ctypes.data_as(ip), int(nslice), b32.ctypes.data_as(ip), int(nbin), int(nboot),
                            None if bidx is None else bidx.ctypes.data_as(_c_int64_p), ctypes.c_uint64(int(seed)), _ptr(phi),
                            _ptr(sums), counts.ctypes.data_as(_c_int64_p))
    if rc != LF_OK:
        raise LFError("lf_veff_slices failed (%d)" % rc)
    return phi, sums, counts


def veff_slices_ms():
    """Device time (ms) of the two kernels of the last lf_veff_slices call in this process (-1 before the first)."""
    return float(load().lf_veff_slices_ms())


def lumfunc_quantiles(variant, draws, logL, z=None, q=(16.0, 50.0, 84.0), method=LF_Q_LINEAR, values=False, device=0):
    """lf_lumfunc_quantiles (include/lfmcmc.h): percentiles over the R draw records `draws` (R x 3, or R x 7 for LF_ZEVOL)
    of the model LF at the P points logL (and z, LF_ZEVOL).  Returns out (nq, P), or (out, values (R, P)) with
    values=True.  method LF_Q_MEDIAN: one row, q ignored.  Raises LFError on a non-zero return."""
    lib = load()
    variant = VARIANTS.get(variant, variant)
    np_rec = 7 if variant == LF_ZEVOL else 3
    draws = _f64(draws).reshape(-1, np_rec)
    logL = _f64(logL).ravel()
    zz = None if z is None else _f64(z).ravel()
    if zz is not None and zz.shape != logL.shape:
        raise ValueError("z must have the shape of logL")
    R, P = draws.shape[0], logL.size
    qa = _f64(np.atleast_1d(q)).ravel() if method == LF_Q_LINEAR else np.zeros(1)
    nq = qa.size
    out = np.empty((nq, P))
    val = np.empty((R, P)) if values else None
    rc = lib.lf_lumfunc_quantiles(int(device), int(variant), R, _ptr(draws), P, _ptr(logL), _ptr(zz), nq, _ptr(qa), int(method),
                                  _ptr(out), _ptr(val))
    if rc != LF_OK:
        raise LFError("lf_lumfunc_quantiles failed (%d)" % rc)
    return (out, val) if values else out


def lumfunc_quantiles_ms():
    """Device time (ms) of the last lf_lumfunc_quantiles kernel in this process (hipEvents around the launch)."""
    ms = np.zeros(1)
    if load().lf_lumfunc_quantiles_ms(_ptr(ms)) != LF_OK:
        raise LFError("no lf_lumfunc_quantiles call has completed")
    return float(ms[0])


def lumfunc_integral_quantiles(variant, kind, draws, logLmin, z=None, q=(16.0, 50.0, 84.0), method=LF_Q_LINEAR, values=False,
                               device=0):
    """lf_lumfunc_integral_quantiles (include/lfmcmc.h): percentiles over the R draw records `draws` (as lumfunc_quantiles
    takes them) of the integrated LF above the P limits logLmin (at z, LF_ZEVOL); kind LF_INT_NUMBER or LF_INT_LUMDENS.
    Returns out (nq, P), or (out, values (R, P)) with values=True.  Raises LFError on a non-zero return."""
    lib = load()
    variant = VARIANTS.get(variant, variant)
    np_rec = 7 if variant == LF_ZEVOL else 3
    draws = _f64(draws).reshape(-1, np_rec)
    logLmin = _f64(logLmin).ravel()
    zz = None if z is None else _f64(z).ravel()
    if zz is not None and zz.shape != logLmin.shape:
        raise ValueError("z must have the shape of logLmin")
    R, P = draws.shape[0], logLmin.size
    qa = _f64(np.atleast_1d(q)).ravel() if method == LF_Q_LINEAR else np.zeros(1)
    nq = qa.size
    out = np.empty((nq, P))
    val = np.empty((R, P)) if values else None
    rc = lib.lf_lumfunc_integral_quantiles(int(device), int(variant), int(kind), R, _ptr(draws), P, _ptr(logLmin), _ptr(zz), nq,
                                           _ptr(qa), int(method), _ptr(out), _ptr(val))
    if rc != LF_OK:
        raise LFError("lf_lumfunc_integral_quantiles failed (%d)" % rc)
    return (out, val) if values else out


def lumfunc_integral_quantiles_ms():
    """Device time (ms) of the last lf_lumfunc_integral_quantiles kernel in this process."""
    ms = np.zeros(1)
    if load().lf_lumfunc_integral_quantiles_ms(_ptr(ms)) != LF_OK:
        raise LFError("no lf_lumfunc_integral_quantiles call has completed")
    return float(ms[0])


def veff_draws_device(flux, field, vol, pref0, fcmin, bin_of, nbin, draws, q=(16.0, 50.0, 84.0), method=LF_Q_LINEAR, device=0):
    """lf_veff_draws (include/lfmcmc.h): the binned 1/Veff sums of the catalogue under each of the R completeness draws
    `draws` (R, nf + 1: Flim per field in erg cm^-2 s^-1, alpha) and their percentiles over the draws.  vol: scalar or
    per-source array.  Returns (out (nq, nbin), values (R, nbin)); method LF_Q_MEDIAN: one row, q ignored.  Raises LFError
    on a non-zero return."""
    lib = load()
    flux = _f64(flux).ravel()
    n = flux.size
    f32 = np.ascontiguousarray(field, dtype=np.int32).ravel()
    b32 = np.ascontiguousarray(bin_of, dtype=np.int32).ravel()
    draws = np.ascontiguousarray(np.atleast_2d(np.asarray(draws, dtype=np.float64)))
    R, nf = draws.shape[0], draws.shape[1] - 1
    volarr = None if np.ndim(vol) == 0 else _f64(vol).ravel()
    if f32.size != n or b32.size != n or (volarr is not None and volarr.size != n):
        raise ValueError("field, bin_of and a per-source vol must have the length of flux")
    qa = _f64(np.atleast_1d(q)).ravel() if method == LF_Q_LINEAR else np.zeros(1)
    nq = qa.size
    out = np.empty((nq, nbin))
    val = np.empty((R, nbin))
    ip = ctypes.POINTER(ctypes.c_int32)
    rc = lib.lf_veff_draws(int(device), n, _ptr(flux), f32.ctypes.data_as(ip), _ptr(volarr), float(vol) if volarr is None else 0.0,
                           float(pref0), float(fcmin) if fcmin else 0.0, b32.ctypes.data_as(ip), int(nbin), int(nf), int(R),
                           _ptr(draws), nq, _ptr(qa), int(method), _ptr(out), _ptr(val))
    if rc != LF_OK:
        raise LFError("lf_veff_draws failed (%d)" % rc)
    return out, val


def veff_draws_zmax_device(flux, field, dist, pref0, fcmin, bin_of, nbin, draws, fmin, table, q=(16.0, 50.0, 84.0), method=LF_Q_LINEAR,
                           device=0):
    """lf_veff_draws_zmax (include/lfmcmc.h): veff_draws_device with the volume of every (source, draw) evaluated on the
    device.  dist: sqrt(L_i / 4 pi) / Mpc_cm per source (veff.source_distance_scale); fmin (R, nf): the flux cut of each draw
    and field in erg cm^-2 s^-1, 0 for none; table: a voltable.VolumeTable.  Returns (out (nq, nbin), values (R, nbin))."""
    lib = load()
    flux = _f64(flux).ravel()
    n = flux.size
    dist = _f64(dist).ravel()
    f32 = np.ascontiguousarray(field, dtype=np.int32).ravel()
    b32 = np.ascontiguousarray(bin_of, dtype=np.int32).ravel()
    draws = np.ascontiguousarray(np.atleast_2d(np.asarray(draws, dtype=np.float64)))
    R, nf = draws.shape[0], draws.shape[1] - 1
    fmin = _f64(fmin).ravel()
    if f32.size != n or b32.size != n or dist.size != n:
        raise ValueError("field, bin_of and dist must have the length of flux")
    if fmin.size != R * nf:
        raise ValueError("fmin must have one value per draw and field")
    head, zc, rec = _f64(table.head).ravel(), _f64(table.zc), _f64(table.rec)
    if head.size != 8 or zc.ndim != 2 or zc.shape[1] != 8 or zc.shape[0] != 32 or rec.ndim != 2 or rec.shape[1] != 8:
        raise ValueError("not a volume table: head (8,), zc (32, 8), rec (K, 8)")
    qa = _f64(np.atleast_1d(q)).ravel() if method == LF_Q_LINEAR else np.zeros(1)
    nq = qa.size
    out = np.empty((nq, nbin))
    val = np.empty((R, nbin))
    ip = ctypes.POINTER(ctypes.c_int32)
    rc = lib.lf_veff_draws_zmax(int(device), n, _ptr(flux), f32.ctypes.data_as(ip), _ptr(dist), float(pref0), float(fcmin) if fcmin else 0.0,
                                b32.ctypes.data_as(ip), int(nbin), int(nf), int(R), _ptr(draws), _ptr(fmin), _ptr(head), _ptr(zc),
                                _ptr(rec), int(rec.shape[0]), nq, _ptr(qa), int(method), _ptr(out), _ptr(val))
    if rc != LF_OK:
        raise LFError("lf_veff_draws_zmax failed (%d)" % rc)
    return out, val


def veff_draws_ms():
    """Device times (ms) of the three stages of the last lf_veff_draws or lf_veff_draws_zmax call in this process:
    per-chunk sums, per-bin sums, quantiles."""
    ms = np.zeros(3)
    if load().lf_veff_draws_ms(_ptr(ms)) != LF_OK:
        raise LFError("no lf_veff_draws call has completed")
    return tuple(float(t) for t in ms)


def veff_draws_chunk():
    """Sources per chunk of lf_veff_draws's summation order."""
    return int(load().lf_veff_draws_chunk())


def gauss_hermite(K):
    """lf_gauss_hermite (include/lfmcmc.h): the library's K-point Gauss-Hermite rule, (x[K] ascending, ln(w_k / sqrt(pi))).
    Touches no GPU."""
    x, lnw = np.empty(int(K)), np.empty(int(K))
    if load().lf_gauss_hermite(int(K), _ptr(x), _ptr(lnw)) != LF_OK:
        raise ValueError("lf_gauss_hermite: K must be in 2..64")
    return x, lnw


def deconv_info():
    """lf_deconv_info: dict orders, sigma_max (per order), default_order, chunk.  Touches no GPU."""
    lib = load()
    n = lib.lf_deconv_info(None, None, 0, None, None)
    orders, smax = np.empty(n, dtype=np.int32), np.empty(n)
    dflt, chunk = ctypes.c_int(0), ctypes.c_int(0)
    lib.lf_deconv_info(orders.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), _ptr(smax), n, ctypes.byref(dflt), ctypes.byref(chunk))
    return {"orders": tuple(int(k) for k in orders), "sigma_max": tuple(float(v) for v in smax), "default_order": int(dflt.value),
            "chunk": int(chunk.value)}


def deconv_wide_info(tables=False):
    """lf_deconv_wide_info: dict edges (the sigma classes' upper edges, dex), nodes (per class), chunk, T, nodes_per_panel, h
    of the wide rule; tables=True: also "tables", per class (x, lnw) in the kernels' form.  Touches no
    GPU."""
    lib = load()
    n = lib.lf_deconv_wide_info(None, None, 0, None, None, None, None, 0, None, None)
    edges, nodes = np.empty(n), np.empty(n, dtype=np.int32)
    chunk, npan = ctypes.c_int(0), ctypes.c_int(0)
    T, h = ctypes.c_double(0.0), ctypes.c_double(0.0)
    lib.lf_deconv_wide_info(_ptr(edges), nodes.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), n, ctypes.byref(chunk), ctypes.byref(T),
                            ctypes.byref(npan), ctypes.byref(h), 0, None, None)
    out = {"edges": tuple(float(v) for v in edges), "nodes": tuple(int(k) for k in nodes), "chunk": int(chunk.value),
           "T": float(T.value), "nodes_per_panel": int(npan.value), "h": float(h.value)}
    if tables:
        tabs = []
        for c in range(n):
            x, lnw = np.empty(out["nodes"][c]), np.empty(out["nodes"][c])
            if lib.lf_deconv_wide_info(None, None, 0, None, None, None, None, c, _ptr(x), _ptr(lnw)) != n:
                raise ValueError("lf_deconv_wide_info: class %d" % c)
            tabs.append((x, lnw))
        out["tables"] = tabs
    return out


def lum_posterior_info():
    """lf_lum_posterior_info: dict row_tile (rows summed in row order before the tiles' sums are added), max_rows.  Touches no
    GPU."""
    rt, mr = ctypes.c_int(0), ctypes.c_int(0)
    load().lf_lum_posterior_info(ctypes.byref(rt), ctypes.byref(mr))
    return {"row_tile": rt.value, "max_rows": mr.value}


def veff_true_info():
    """lf_veff_true_info: dict max_rows, max_bins, row_group (the rows of one launch group: the workspace's height).  Touches no
    GPU."""
    mr, mb = ctypes.c_int(0), ctypes.c_int(0)
    rg = load().lf_veff_true_info(ctypes.byref(mr), ctypes.byref(mb))
    return {"max_rows": mr.value, "max_bins": mb.value, "row_group": rg}


def veff_true_ms():
    """lf_veff_true_ms: the device milliseconds (node kernel, chunk sums, quantiles) of the last lf_veff_true call"""
    ms = np.zeros(3)
    if load().lf_veff_true_ms(_ptr(ms)) != LF_OK:
        raise RuntimeError("lf_veff_true_ms: no successful lf_veff_true call yet")
    return ms


def _ptr(a):
    return a.ctypes.data_as(_c_double_p) if a is not None else None


def log_flux(lum, dl_mpc):
    """logf_i = lum_i - log10(4 pi (3.086e24 DLf(z_i))^2): log10 of the flux of lumfuncmcmc.py:70."""
    return np.asarray(lum, dtype=np.float64) - np.log10(4.0 * np.pi * (MPC_CM * np.asarray(dl_mpc, dtype=np.float64)) ** 2)


class LFError(RuntimeError):
    pass


class LFContext(object):
    """One catalogue + grids resident on one MI355X.  `inp` uses the reference's own names
    (the attributes LumFuncMCMC / LumFuncMCMCz build in __init__):

        variant, fix_sch_al, sch_al0, field_ind, lum, DLz | logf, z, Om_arr, Omega_0, Flim0, alpha0,
        logL (S,S), zarr, volume_part, DL_zarr, integ_part (nf,S,S) | integ_sum (S,S), fcmin,
        lims {Lstar, phistar, sch_al, Flim, alpha}, pivots
    """

    def __init__(self, inp, device=0, max_batch=0):
        lib = load()
        self._lib = lib
        self._h = None
        variant = inp["variant"]
        if variant not in VARIANTS:
            raise ValueError("variant must be one of %s" % (sorted(VARIANTS),))
        self.variant = variant
        fi = np.ascontiguousarray(inp["field_ind"], dtype=np.int64)
        nf = len(fi) - 1
        lum = _f64(inp["lum"])
        N = lum.shape[0]
        logL = _f64(inp["logL"])
        S = logL.shape[0]
        if logL.shape != (S, S):
            raise ValueError("logL must be (S, S)")
        keep = {"fi": fi, "lum": lum, "logL": logL, "zarr": _f64(inp["zarr"]),
                "omega0": _f64(inp["Omega_0"])}
        d = LfDesc()
        d.variant = VARIANTS[variant]
        d.fix_sch_al = 1 if inp.get("fix_sch_al", False) else 0
        d.nf, d.S, d.N = nf, S, N
        if variant == "free":
            if inp.get("logf") is not None:
                keep["logf"] = _f64(inp["logf"])
            else:
                keep["logf"] = _f64(log_flux(lum, inp["DLz"]))
            keep["volume_part"] = _f64(inp["volume_part"])
            keep["dl_zarr"] = _f64(inp["DL_zarr"])
        else:
            keep["om_arr"] = _f64(inp["Om_arr"])
            ip = inp.get("integ_part")
            if ip is None:        # a field-summed table: field 0 carries the sum, the rest are zero
                ip = np.zeros((nf, S, S))
                ip[0] = inp["integ_sum"]
            keep["integ_part"] = _f64(ip)
            if keep["integ_part"].shape != (nf, S, S):
                raise ValueError("integ_part must be (nf, S, S)")
            if variant == "zevol":
                keep["z"] = _f64(inp["z"])
            else:
                keep["flim0"] = _f64(inp["Flim0"])
                d.alpha0 = float(inp["alpha0"])
            # (read by lf_set_cut_error_model alone: the columns' volume element and distance)
            if inp.get("volume_part") is not None and inp.get("DL_zarr") is not None:
                keep["volume_part"] = _f64(inp["volume_part"])
                keep["dl_zarr"] = _f64(inp["DL_zarr"])
        for k in ("logf", "z", "om_arr", "volume_part", "dl_zarr", "integ_part", "flim0"):
            setattr(d, k, _ptr(keep.get(k)))
        d.field_ind = fi.ctypes.data_as(_c_int64_p)
        d.lum = _ptr(lum)
        d.omega0 = _ptr(keep["omega0"])
        d.logL = _ptr(logL)
        d.zarr = _ptr(keep["zarr"])
        d.sch_al0 = float(inp.get("sch_al0", 0.0))
        d.fcmin = float(inp.get("fcmin", 0.1))
        lims = inp["lims"]
        for i, name in enumerate(LIM_ORDER):
            d.lims[i][0], d.lims[i][1] = float(lims[name][0]), float(lims[name][1])
        piv = inp.get("pivots", (1.20, 1.53, 1.86))
        for i in range(3):
            d.pivots[i] = float(piv[i])
        d.device = int(device)
        d.max_batch = int(max_batch)
        h = lib.lf_create(ctypes.byref(d))
        if not h:
            raise LFError(lib.lf_last_error(None).decode())
        self._h = ctypes.c_void_p(h)
        self.ndim = lib.lf_ndim(self._h)
        self.N, self.nf, self.S = N, nf, S
        self.fix_sch_al = bool(d.fix_sch_al)
        self.lims = {k: (float(lims[k][0]), float(lims[k][1])) for k in LIM_ORDER}
        self.device = int(device)
        # what lf_set_lum_err needs beyond sigma for fixed completeness: the sources' log flux and the fixed curve
        self._logf = keep["logf"] if variant == "free" else (_f64(inp["logf"]) if inp.get("logf") is not None else
                                                             (_f64(log_flux(lum, inp["DLz"])) if inp.get("DLz") is not None else None))
        self._flim0 = None if variant == "free" else _f64(inp["Flim0"])
        self._alpha0 = 0.0 if variant == "free" else float(inp["alpha0"])

    def prior_box(self):
        """(ndim, 2) bounds of the flat prior in theta's order (the model classes' _theta_lims)."""
        L = self.lims
        if self.variant == "zevol":
            rows = [L["Lstar"]] * 3 + [L["phistar"]] * 3
        else:
            rows = [L["Lstar"], L["phistar"]]
        if not self.fix_sch_al:
            rows.append(L["sch_al"])
        if self.variant == "free":
            rows += [L["Flim"]] * self.nf + [L["alpha"]]
        box = np.array(rows, dtype=np.float64)
        assert box.shape == (self.ndim, 2), (box.shape, self.ndim)
        return box

    # ------------------------------------------------------------------ calls
    def _check(self, rc):
        if rc != LF_OK:
            raise LFError("liblfmcmc error %d: %s" % (rc, self._lib.lf_last_error(self._h).decode()))

    def _theta(self, theta):
        th = np.ascontiguousarray(np.atleast_2d(np.asarray(theta, dtype=np.float64)))
        if th.ndim != 2 or th.shape[1] != self.ndim:
            raise ValueError("theta must be (B, %d), got %s" % (self.ndim, th.shape))
        return th

    def _value_grad(self, fn, theta):
        """A "(value, gradient)" call of the library on host arrays: fn(handle, theta, B, value (B,), grad (B, ndim))."""
        th = self._theta(theta)
        lp = np.empty(th.shape[0], dtype=np.float64)
        g = np.empty((th.shape[0], self.ndim), dtype=np.float64)
        if th.shape[0]:
            self._check(fn(self._h, _ptr(th), th.shape[0], _ptr(lp), _ptr(g)))
        return lp, g

    def _device_theta(self, theta):
        """Checks a float64 device tensor (B, ndim) on this context's device -> (it, contiguous; B; torch's current stream)."""
        import torch
        if theta.dtype != torch.float64 or not theta.is_cuda or theta.dim() != 2 or theta.shape[1] != self.ndim:
            raise ValueError("theta must be a float64 device tensor of shape (B, %d)" % self.ndim)
        if theta.device.index != self.device:
            raise ValueError("theta is on device %s, context is on %d" % (theta.device, self.device))
        return theta.contiguous(), theta.shape[0], torch.cuda.current_stream(theta.device).cuda_stream

    def _value_grad_torch(self, fn, theta):
        """The same on device tensors, enqueued on torch's current stream: fn(handle, theta, B, value, grad, stream)."""
        import torch
        theta, B, stream = self._device_theta(theta)
        lp = torch.empty(B, dtype=torch.float64, device=theta.device)
        g = torch.empty((B, self.ndim), dtype=torch.float64, device=theta.device)
        if B:
            self._check(fn(self._h, ctypes.c_void_p(theta.data_ptr()), int(B), ctypes.c_void_p(lp.data_ptr()),
                           ctypes.c_void_p(g.data_ptr()), ctypes.c_void_p(stream)))
        return lp, g

    def lnprob_batch(self, theta):
        """theta (B, ndim) or (ndim,) host array -> lnprob (B,) float64."""
        th = self._theta(theta)
        out = np.empty(th.shape[0], dtype=np.float64)
        if th.shape[0] == 0:
            return out
        self._check(self._lib.lf_lnprob_batch(self._h, _ptr(th), th.shape[0], _ptr(out)))
        return out

    def lnprob_pieces(self, theta):
        th = self._theta(theta)
        a = np.empty(th.shape[0], dtype=np.float64)
        b = np.empty(th.shape[0], dtype=np.float64)
        if th.shape[0] == 0:
            return a, b
        self._check(self._lib.lf_lnprob_pieces(self._h, _ptr(th), th.shape[0], _ptr(a), _ptr(b)))
        return a, b

    def lnprob_grad(self, theta):
        """theta (B, ndim) or (ndim,) host array -> (lnprob (B,), grad (B, ndim)): lf_lnprob_grad_batch.  lnprob is
        lnprob_batch's, bit for bit; rows whose lnprob is -inf have NaN gradients."""
        return self._value_grad(self._lib.lf_lnprob_grad_batch, theta)

    def set_lum_err(self, sigma, K=None, unchecked=False, wide=False):
        """lf_set_lum_err: the sources' luminosity errors sigma (dex, catalogue order) and the Gauss-Hermite order K (None: the
        library's default) of the flux-error-convolved likelihood (lnprob_err_batch).  unchecked=True
        sets the option "deconv_unchecked" first: sigma above the order's validated range is taken as it is.  wide=True sets
        the option "deconv_wide" first: sigma above that range, up to 0.30 dex, goes to the wide rule."""
        sg = _f64(sigma).ravel()
        if sg.size != self.N:
            raise ValueError("sigma must have one value per source (%d), got %d" % (self.N, sg.size))
        if K is None:
            K = deconv_info()["default_order"]
        if self.variant != "free" and self._logf is None:
            raise ValueError("set_lum_err: the inputs of a fixed-completeness context must hold logf or DLz")
        self.set_option("deconv_unchecked", 1 if unchecked else 0)
        self.set_option("deconv_wide", 1 if wide else 0)
        self._check(self._lib.lf_set_lum_err(self._h, _ptr(sg), int(K), None if self.variant == "free" else _ptr(self._logf),
                                             _ptr(self._flim0), float(self._alpha0)))
        self.deconv_order = int(K)

    def set_cut_error_model(self, nodes, sigma):
        """lf_set_cut_error_model: the error model sigma (nf, M) in dex at the log10 flux nodes (M,) of the cut on the observed
        flux, on a context whose grid has its own luminosity nodes per column (min_comp_frac > 0.001).
        Before set_lum_err, which then accepts such a context; lnprob_err_batch and the device samplers' convolved likelihood
        then hold lnprob + Delta - Delta B."""
        nd = _f64(nodes).ravel()
        sg = np.ascontiguousarray(np.atleast_2d(np.asarray(sigma, dtype=np.float64)))
        if sg.shape != (self.nf, nd.size):
            raise ValueError("sigma must be (nf, M) = (%d, %d), got %s" % (self.nf, nd.size, sg.shape))
        self._check(self._lib.lf_set_cut_error_model(self._h, _ptr(nd), int(nd.size), _ptr(sg)))

    def cut_term_batch(self, theta):
        """theta (B, ndim) or (ndim,) host array -> Delta B (B,), the cut's change of the expected counts: lf_cut_term_batch
        (NaN for a row whose plain lnprob is not finite).  Needs set_cut_error_model and set_lum_err."""
        th = self._theta(theta)
        out = np.empty(th.shape[0], dtype=np.float64)
        if th.shape[0]:
            self._check(self._lib.lf_cut_term_batch(self._h, _ptr(th), th.shape[0], _ptr(out)))
        return out

    def cut_term_grad(self, theta):
        """theta (B, ndim) or (ndim,) host array -> (Delta B (B,), d Delta B / d theta (B, ndim)): lf_cut_term_grad_batch.  Delta
        B is cut_term_batch's, bit for bit; a row whose plain lnprob is not finite has NaN throughout.
        Served whatever the option "deconv_cut_grad" says."""
        return self._value_grad(self._lib.lf_cut_term_grad_batch, theta)

    def cut_info(self):
        """lf_cut_info: dict nnodes (nf,), H (nf,), chunk (nodes per block), chunks (blocks per row; -1 before the tables are made)."""
        n = np.zeros(self.nf, dtype=np.int32)
        H = np.zeros(self.nf)
        chunk, chunks = ctypes.c_int(0), ctypes.c_int(0)
        rc = self._lib.lf_cut_info(self._h, n.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), _ptr(H), self.nf, ctypes.byref(chunk),
                                   ctypes.byref(chunks))
        if rc < 0:
            self._check(rc)
        return {"nnodes": n, "H": H, "chunk": chunk.value, "chunks": chunks.value}

    def lnprob_err_batch(self, theta):
        """theta (B, ndim) or (ndim,) host array -> the flux-error-convolved lnprob (B,): lf_lnprob_err_batch."""
        th = self._theta(theta)
        out = np.empty(th.shape[0], dtype=np.float64)
        if th.shape[0]:
            self._check(self._lib.lf_lnprob_err_batch(self._h, _ptr(th), th.shape[0], _ptr(out)))
        return out

    def lum_posterior(self, theta):
        """theta (R, ndim) or (ndim,) host array, 1 <= R <= 4096 -> (m1 (N,), m2 (N,), n_used): lf_lum_posterior, the per-source
        posterior mean and second moment of (true - catalogued) log-luminosity under the convolved model, averaged over the
        rows whose plain lnprob is finite, in catalogue order.  Needs set_lum_err."""
        th = self._theta(theta)
        m1, m2 = np.empty(self.N, dtype=np.float64), np.empty(self.N, dtype=np.float64)
        used = ctypes.c_int(0)
        self._check(self._lib.lf_lum_posterior(self._h, _ptr(th), th.shape[0], _ptr(m1), _ptr(m2), ctypes.byref(used)))
        return m1, m2, used.value

    def veff_true(self, theta, edges, pref0, vol, q=(16.0, 50.0, 84.0), method=LF_Q_LINEAR, min_vol_frac=0.0):
        """theta (R, ndim) or (ndim,) host array, 1 <= R <= 4096; edges (nbin + 1,) ascending -> (out (nq, nbin), values
        (R, nbin), n_used): lf_veff_true, the deconvolved 1/Veff points - every source's posterior of the true luminosity
        binned with the completeness at the node's true flux, per row (NaN for a row whose plain lnprob is not finite), and
        NumPy's percentiles q of every bin over the used rows.  method LF_Q_MEDIAN: one row of out, q
        ignored.  Needs set_lum_err.  On a context with the cut model and the option "deconv_cut_veff" every node's weight is
        divided by its catalogued volume fraction g, and a node with g = 0 or g < min_vol_frac is dropped (lf_veff_true_cut;
        DESIGN.md section 3.34)."""
        th = self._theta(theta)
        ed = _f64(edges).ravel()
        nbin = ed.size - 1
        qa = _f64(np.atleast_1d(q)).ravel() if method == LF_Q_LINEAR else np.zeros(1)
        nq = qa.size if method == LF_Q_LINEAR else 1
        out = np.empty((nq, max(nbin, 0)), dtype=np.float64)
        values = np.empty((th.shape[0], max(nbin, 0)), dtype=np.float64)
        used = ctypes.c_int(0)
        if min_vol_frac == 0.0:
            self._check(self._lib.lf_veff_true(self._h, _ptr(th), th.shape[0], _ptr(ed), nbin, float(pref0), float(vol), nq, _ptr(qa),
                                               int(method), _ptr(out), _ptr(values), ctypes.byref(used)))
        else:
            self._check(self._lib.lf_veff_true_cut(self._h, _ptr(th), th.shape[0], _ptr(ed), nbin, float(pref0), float(vol),
                                                   float(min_vol_frac), nq, _ptr(qa), int(method), _ptr(out), _ptr(values),
                                                   ctypes.byref(used)))
        return out, values, used.value

    def veff_true_cut_info(self):
        """lf_veff_true_cut_info: dict slots, bytes, dropped of the table of catalogued volumes the last veff_true call under
        the cut made or reused, and ms, the device time of the kernel that made it."""
        sl, by, dr = (np.zeros(1, dtype=np.int64) for _ in range(3))
        ms = np.zeros(1)
        self._check(self._lib.lf_veff_true_cut_info(self._h, sl.ctypes.data_as(_c_int64_p), by.ctypes.data_as(_c_int64_p),
                                                    dr.ctypes.data_as(_c_int64_p)))
        self._check(self._lib.lf_veff_true_cut_ms(self._h, _ptr(ms)))
        return {"slots": int(sl[0]), "bytes": int(by[0]), "dropped": int(dr[0]), "ms": float(ms[0])}

    def cut_volume(self, field, L):
        """field (n,) or a scalar, L (n,) -> g (n,): lf_cut_volume, the part of the survey volume in which a true luminosity L of
        the field is catalogued under the cut (deconv.cut_volume_fraction's statements on the device).  Needs
        set_cut_error_model."""
        Lq = _f64(np.atleast_1d(L)).ravel()
        fq = np.ascontiguousarray(np.broadcast_to(np.asarray(field, dtype=np.int32), Lq.shape))
        g = np.empty(Lq.size, dtype=np.float64)
        self._check(self._lib.lf_cut_volume(self._h, fq.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), _ptr(Lq), Lq.size, _ptr(g)))
        return g

    def lnprob_err_torch(self, theta):
        """theta: float64 device tensor (B, ndim) on this context's device; enqueues lf_lnprob_err_batch_device on torch's
        current stream and returns a (B,) device tensor."""
        import torch
        theta, B, stream = self._device_theta(theta)
        out = torch.empty(B, dtype=torch.float64, device=theta.device)
        if B:
            self._check(self._lib.lf_lnprob_err_batch_device(self._h, ctypes.c_void_p(theta.data_ptr()), int(B),
                                                             ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(stream)))
        return out

    def lnprob_err_grad(self, theta):
        """theta (B, ndim) or (ndim,) host array -> (lnprob_err (B,), grad (B, ndim)): lf_lnprob_err_grad_batch.  The value is
        lnprob_err_batch's, bit for bit; rows whose plain lnprob is not finite have NaN gradients."""
        return self._value_grad(self._lib.lf_lnprob_err_grad_batch, theta)

    def lnprob_err_grad_torch(self, theta):
        """theta: float64 device tensor (B, ndim) on this context's device; enqueues lf_lnprob_err_grad_batch_device on torch's
        current stream and returns (lnprob_err (B,), grad (B, ndim)) device tensors."""
        return self._value_grad_torch(self._lib.lf_lnprob_err_grad_batch_device, theta)

    def lnprob_grad_torch(self, theta):
        """theta: float64 device tensor (B, ndim) on this context's device; enqueues lf_lnprob_grad_batch_device on torch's
        current stream and returns (lnprob (B,), grad (B, ndim)) device tensors."""
        return self._value_grad_torch(self._lib.lf_lnprob_grad_batch_device, theta)

    def lnprob_batch_device(self, theta_ptr, B, out_ptr, stream=0):
        """Raw device pointers (ints) and a hipStream_t handle (int, 0 = default stream)."""
        self._check(self._lib.lf_lnprob_batch_device(self._h, ctypes.c_void_p(theta_ptr), int(B),
                                                     ctypes.c_void_p(out_ptr), ctypes.c_void_p(stream)))

    def lnprob_torch(self, theta, out=None):
        """theta: CUDA(=HIP) float64 tensor (B, ndim) on this context's device; enqueues on
        torch's current stream and returns a (B,) tensor.  torch is plumbing here: device memory
        and streams only."""
        import torch
        theta, B, stream = self._device_theta(theta)
        if out is None:
            out = torch.empty(B, dtype=torch.float64, device=theta.device)
        if B:
            self.lnprob_batch_device(theta.data_ptr(), B, out.data_ptr(), stream)
        return out

    def lnprob_torch_n(self, theta, out=None):
        """K independent blocks in one C call (lf_lnprob_batch_device_n): theta (K, B, ndim) device tensor -> (K, B)."""
        import torch
        if theta.dtype != torch.float64 or not theta.is_cuda or theta.dim() != 3 or theta.shape[2] != self.ndim:
            raise ValueError("theta must be a float64 device tensor of shape (K, B, %d)" % self.ndim)
        theta = theta.contiguous()
        K, B = theta.shape[0], theta.shape[1]
        if out is None:
            out = torch.empty((K, B), dtype=torch.float64, device=theta.device)
        if K and B:
            stream = torch.cuda.current_stream(theta.device).cuda_stream
            self._check(self._lib.lf_lnprob_batch_device_n(self._h, ctypes.c_void_p(theta.data_ptr()), int(B), int(K),
                                                           ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(stream)))
        return out

    def set_profiling(self, level):
        """0 off, 1 the main kernel only, 2 every launch (True = 2)."""
        self._check(self._lib.lf_set_profiling(self._h, 2 if level is True else int(level)))

    def kernel_times(self):
        ms = (ctypes.c_double * 4)()
        n = (ctypes.c_int64 * 4)()
        self._check(self._lib.lf_kernel_times(self._h, ms, n))
        names = ("prepare", "main", "unused", "finalize")
        return {k: {"ms": ms[i], "launches": int(n[i])} for i, k in enumerate(names)}

    FORM_NAMES = ("general", "general_noexp", "table", "table_noexp", "careful", "skipped", "node_general", "node_bright", "cell")

    def form_counts(self):
        """Census of the term forms since set_option("count_forms", 1): dict name -> count (include/lfmcmc.h)."""
        n = (ctypes.c_int64 * 9)()
        self._check(self._lib.lf_form_counts(self._h, n))
        return {k: int(n[i]) for i, k in enumerate(self.FORM_NAMES)}

    def last_launch(self):
        """Shape of the most recent lf_main launch: dict st, tw, twb, compressed, workgroups, chunks_a, chunks_b, rows."""
        n = (ctypes.c_int32 * 8)()
        self._check(self._lib.lf_last_launch(self._h, n))
        d = dict(zip(("st", "tw", "twb", "kind", "workgroups", "chunks_a", "chunks_b", "rows"), (int(v) for v in n)))
        d["compressed"] = int(d["kind"] == 1)
        d["fused"] = d["kind"] in (3, 5)            # lf_free / lf_pers doing lf_prepare's and lf_finalize's work too: one launch
        if d["fused"]:
            d["kind"] -= 1
        d["kernel"] = "lf_free<%d>" % d["st"] if d["kind"] == 2 else ("lf_pers" if d["kind"] == 4 else "lf_main")
        if d["kind"] in (2, 4):                     # the persistent kernels: groups of 8 workgroups, group k on tiles k % ntiles, + tile_stride, ...
            d["tile_stride"] = d["workgroups"] // 8
        return d

    def free_block_uploads(self):
        """Uploads of the one-launch lf_free's argument block so far (lf_free.h: FreeBlock; none in steady state)."""
        n = ctypes.c_int64(0)
        self._check(self._lib.lf_free_block_uploads(self._h, ctypes.byref(n)))
        return int(n.value)

    def set_option(self, key, value):
        self._check(self._lib.lf_set_option(self._h, key.encode(), int(value)))

    def close(self):
        if self._h is not None:
            self._lib.lf_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
