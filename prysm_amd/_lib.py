"""ctypes binding of libprysm_amd.so (the C ABI in include/prysm_amd.h).

There is no CPU fallback: if the shared library is missing, or no MI355X is
visible, every compute call raises.  PyTorch is used only as the owner of
device memory and streams; all arithmetic on the hot path happens in the HIP
kernels behind this binding.
"""
import ctypes
import threading
import os

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# PRYSM_AMD_LIB: another BUILD of the same library (tools/exp_ab_libs.py: two builds -- e.g. two commits -- against each other on one box)
LIB_PATH = os.environ.get('PRYSM_AMD_LIB') or os.path.join(_HERE, 'libprysm_amd.so')

PM_C64, PM_C128, PM_F32, PM_F64, PM_BOOL = 0, 1, 2, 3, 4
PM_U8, PM_U16, PM_U32 = 5, 6, 7
PM_EPI_NONE, PM_EPI_ABS2, PM_EPI_ABS2_ACCUM, PM_EPI_ABS, PM_EPI_ARG = 0, 1, 2, 3, 4
PM_MUL_NONE, PM_MUL_FULL, PM_MUL_SEPARABLE = 0, 1, 2
PM_FLAG_PASS1_ONLY, PM_FLAG_PASS2_ONLY, PM_FLAG_REAL_INPUT, PM_FLAG_SYNTH_INPUT, PM_FLAG_NORM_DC, PM_FLAG_SYNTH_PACKED = 1, 2, 4, 8, 16, 32
PM_FLAG_REAL_OUTPUT = 64
PM_ERR_ARG, PM_ERR_UNSUPPORTED, PM_ERR_WORKSPACE = -1, -2, -3
PM_LATTICE_SCATTER, PM_LATTICE_GATHER = 0, 1
PM_ZERNIKE_CARTESIAN, PM_ZERNIKE_POLAR = 0, 1
PM_QPOLY_RADIAL = 2
PM_RECUR_X, PM_RECUR_R2 = 0, 1
PM_RECUR2_Z, PM_RECUR2_ZX, PM_RECUR2_ZY = 1, 2, 4
PM_SEGMENT_ZERNIKE, PM_SEGMENT_STORED = 0, 1
PM_COORDS_GRID, PM_COORDS_SEPARABLE, PM_COORDS_POINTWISE = 0, 1, 2
PM_SDF_MASK, PM_SDF_DISTANCE, PM_SDF_COVERAGE = 0, 1, 2
PM_BIN_AVG, PM_BIN_SUM = 0, 1
PM_CFA_RGGB, PM_CFA_BGGR = 0, 1
PM_BAYER_COMPOSITE, PM_BAYER_RECOMPOSITE = 0, 1
PM_BAYER_MOSAIC, PM_BAYER_RGB = 0, 1
PM_COST_MSE, PM_COST_BGI, PM_COST_NLL = 0, 1, 2
PM_LBFGSB_MAX_MEMORY, PM_LBFGSB_TILE, PM_LBFGSB_THREADS, PM_LBFGSB_WGS, PM_LBFGSB_GRAM_WGS = 32, 8, 256, 1024, 256
PM_LBFGSB_DIRECTION, PM_LBFGSB_RESIDUAL, PM_LBFGSB_SUBSPACE = 0, 1, 2
PM_LBFGSB_SMALL_DIRECTION, PM_LBFGSB_SMALL_BREAK, PM_LBFGSB_SMALL_RESIDUAL, PM_LBFGSB_SMALL_SUBSPACE, PM_LBFGSB_SMALL_UPDATE = 0, 1, 2, 3, 4
PM_OPT_GD, PM_OPT_ADAGRAD, PM_OPT_RMSPROP, PM_OPT_ADAM, PM_OPT_RADAM, PM_OPT_ADAMOMENTUM, PM_OPT_YOGI = 0, 1, 2, 3, 4, 5, 6
PM_ACT_TANH, PM_ACT_ARCTAN, PM_ACT_SOFTPLUS, PM_ACT_SIGMOID = 0, 1, 2, 3
PM_GRAD_FORWARD_X, PM_GRAD_ADJOINT_X, PM_GRAD_FORWARD_Y, PM_GRAD_ADJOINT_Y = 0, 1, 2, 3
PM_TF_S, PM_TF_P, PM_TF_BOTH = 0, 1, 2
PM_TF_T_STACK, PM_TF_T_THINFILM = 0, 1
PM_RT_REFLECT, PM_RT_REFRACT, PM_RT_MEASURE = 0, 1, 2
PM_RT_PLANE, PM_RT_CONIC, PM_RT_ASPHERE = 0, 1, 2
PM_RT_OK, PM_RT_NEWTON, PM_RT_CLIP, PM_RT_MISS, PM_RT_TIR = 0, 1, 2, -1, -2
PM_RT_RECORD, PM_RT_MAX_SURFACES, PM_RT_MAX_COEFS = 48, 4096, 8
PM_OBJECT_SLIT, PM_OBJECT_PINHOLE, PM_OBJECT_SIEMENSSTAR, PM_OBJECT_TILTEDSQUARE, PM_OBJECT_SLANTEDEDGE = 0, 1, 2, 3, 4
PM_OBJECT_SLIT_X, PM_OBJECT_SLIT_Y, PM_OBJECT_BINARY, PM_OBJECT_CROSSED = 1, 2, 4, 8
(PM_TFP_SINC_X, PM_TFP_SINC_Y, PM_TFP_COS_X, PM_TFP_COS_Y, PM_TFP_GAUSS_R, PM_TFP_JINC_R, PM_TFP_AIRY_FT_R, PM_TFP_SLIT_FT, PM_TFP_MAP_REAL,
 PM_TFP_MAP_COMPLEX, PM_TFP_AIRY_R, PM_TFP_AIRY_EFIELD_R) = range(12)
PM_FREQ_GRID, PM_FREQ_VECTORS, PM_FREQ_POINTWISE = 0, 1, 2
PM_TF_MAX_RECORDS = 16
PM_PSI_MAX_FRAMES = 32
PM_LENSLET_RECTANGLE, PM_LENSLET_CIRCLE = 0, 1
PM_GRATING_SIN_AMP, PM_GRATING_PULSE = 0, 1
(PM_IFG_N, PM_IFG_NNAN, PM_IFG_SUM, PM_IFG_SUMSQ, PM_IFG_MIN, PM_IFG_MAX, PM_IFG_ROW0, PM_IFG_ROW1, PM_IFG_COL0, PM_IFG_COL1, PM_IFG_MEAN,
 PM_IFG_SAD, PM_IFG_M2, PM_IFG_STD, PM_IFG_RMS, PM_IFG_SA, PM_IFG_RECORD) = range(17)
PM_IFG_TERM_PISTON, PM_IFG_TERM_X, PM_IFG_TERM_Y, PM_IFG_TERM_R2 = 1, 2, 4, 8
PM_IFG_FILL, PM_IFG_MASK, PM_IFG_CLIP = 0, 1, 2
PM_IFG_WIN_WELCH, PM_IFG_WIN_HANN, PM_IFG_WIN_ARRAY = 0, 1, 2
PM_IFG_LP, PM_IFG_HP, PM_IFG_BP, PM_IFG_BR = 0, 1, 2, 3
PM_IFG_PSD_ABC, PM_IFG_PSD_AB = 0, 1
PM_IFG_IIR_HANN, PM_IFG_IIR_LPF = 1, 2
PM_PSD_MASK_NONE, PM_PSD_MASK_ARRAY, PM_PSD_MASK_CIRCLE = 0, 1, 2
PM_JONES_AOS, PM_JONES_PLANES = 0, 1
PM_JONES_ROTATION, PM_JONES_RETARDER, PM_JONES_DIATTENUATOR, PM_JONES_VORTEX, PM_JONES_LINPOL_VECTOR = range(5)
PM_JONES_FIELD_NONE, PM_JONES_FIELD_REAL, PM_JONES_FIELD_COMPLEX = 0, 1, 2
PM_JONES_LEAKAGE_IDENTITY, PM_JONES_MAX_CHAIN = 1, 6
PM_MODES_FIT_MAX = 128
PM_MODES_REC_COUNT, PM_MODES_REC_RANK, PM_MODES_REC_G = 0, 1, 2
PM_MODES_GRAM, PM_MODES_RHS = 1, 2
PM_MODES_FACTOR, PM_MODES_SOLVE, PM_MODES_INVERT, PM_MODES_NORMS_STD, PM_MODES_NORMS_PTP = 0, 1, 2, 3, 4
PM_MODES_LOWER, PM_MODES_DIAGONAL = 0, 1
(PM_MODES_STAT_N, PM_MODES_STAT_SUM, PM_MODES_STAT_MIN, PM_MODES_STAT_MAX, PM_MODES_STAT_MEAN, PM_MODES_STAT_M2, PM_MODES_STAT_STD,
 PM_MODES_STAT_RECORD) = range(8)

c_i32, c_i64, c_f64, c_vp, c_sz = ctypes.c_int32, ctypes.c_int64, ctypes.c_double, ctypes.c_void_p, ctypes.c_size_t


class pm_axis(ctypes.Structure):
    _fields_ = [('n', c_i64), ('len', c_i64), ('off', c_i64), ('shift', c_i64)]


class pm_fft2_desc(ctypes.Structure):
    _fields_ = [
        ('dtype', c_i32), ('direction', c_i32), ('epilogue', c_i32), ('flags', c_i32),
        ('scale', c_f64), ('weight', c_f64),
        ('in_y', pm_axis), ('in_x', pm_axis), ('out_y', pm_axis), ('out_x', pm_axis),
        ('in_ld', c_i64), ('out_ld', c_i64),
        ('mul_kind', c_i32), ('mul_conj', c_i32), ('mul', c_vp), ('mul_x', c_vp), ('mul_ld', c_i64),
        ('batch', c_i64), ('in_bstride', c_i64), ('out_bstride', c_i64), ('mul_bstride', c_i64), ('mul_x_bstride', c_i64),
        ('synth_amp', c_vp), ('synth_amp_dtype', c_i32), ('synth_reserved', c_i32), ('synth_amp_ld', c_i64), ('synth_k', c_f64),
    ]


class pm_object(ctypes.Structure):
    _fields_ = [('kind', c_i32), ('flags', c_i32), ('p', c_f64 * 8)]


class pm_tf_record(ctypes.Structure):
    _fields_ = [('kind', c_i32), ('flags', c_i32), ('ld', c_i64), ('ptr', c_vp), ('p', c_f64 * 4)]


class pm_tf_freq(ctypes.Structure):
    _fields_ = [('mode', c_i32), ('shift', c_i32), ('dx', c_f64), ('fx', c_vp), ('fy', c_vp), ('fr', c_vp), ('ldx', c_i64), ('ldy', c_i64),
                ('ldr', c_i64)]


class pm_psi_frames(ctypes.Structure):
    _fields_ = [('frame', c_vp * PM_PSI_MAX_FRAMES), ('s', c_f64 * PM_PSI_MAX_FRAMES), ('c', c_f64 * PM_PSI_MAX_FRAMES)]


class pm_lenslets(ctypes.Structure):
    _fields_ = [('kind', c_i32), ('nx', c_i32), ('ny', c_i32), ('reserved', c_i32), ('pitch', c_f64), ('shift_x', c_f64), ('shift_y', c_f64),
                ('half_width', c_f64), ('half_height', c_f64), ('efl', c_f64), ('k', c_f64)]


class pm_ifg_coords(ctypes.Structure):
    _fields_ = [('mode', c_i32), ('linspace', c_i32), ('x', c_vp), ('y', c_vp), ('ldx', c_i64), ('ldy', c_i64), ('ox', c_i64), ('oy', c_i64),
                ('dx', c_f64), ('dy', c_f64), ('x0', c_f64), ('y0', c_f64)]


class pm_psd_model(ctypes.Structure):
    _fields_ = [('kind', c_i32), ('reserved', c_i32), ('a', c_f64), ('b', c_f64), ('c', c_f64), ('dxg', c_f64)]


class pm_jones_param(ctypes.Structure):
    _fields_ = [('value', c_f64), ('map', c_vp), ('ld', c_i64)]


class pm_jones_optic_desc(ctypes.Structure):
    _fields_ = [('kind', c_i32), ('flags', c_i32), ('charge', c_f64), ('p', pm_jones_param * 3)]


class pm_jones_operand(ctypes.Structure):
    _fields_ = [('map', c_vp), ('ld', c_i64), ('pstride', c_i64), ('c', c_f64 * 8)]


# name -> (restype, argtypes); tests/test_capi_symbols.py checks this table against include/prysm_amd.h
SIGNATURES = {
    'pm_version': (c_i32, []),
    'pm_last_error': (ctypes.c_char_p, []),
    'pm_plan_prepare': (c_i32, [c_i32, c_i64]),
    'pm_shutdown': (None, []),
    'pm_set_tuning': (c_i32, [ctypes.c_char_p, c_i32]),
    'pm_set_tuning_local': (c_i32, [ctypes.c_char_p, c_i32]),
    'pm_reset_tuning_local': (None, []),
    'pm_plan_explain': (c_i32, [ctypes.POINTER(pm_fft2_desc), c_i32, ctypes.c_char_p, c_sz]),
    'pm_r2c_untangle': (c_i32, [c_i32, c_i64, c_i64, c_vp, c_i64, c_i64, c_i64, c_i64, c_i64, c_i32, c_i32, c_f64, c_vp, c_i64, c_vp]),
    'pm_fft2_workspace': (c_sz, [ctypes.POINTER(pm_fft2_desc)]),
    'pm_fft2': (c_i32, [ctypes.POINTER(pm_fft2_desc), c_vp, c_vp, c_vp, c_sz, c_vp]),
    'pm_fft2_spectral_workspace': (c_sz, [ctypes.POINTER(pm_fft2_desc), c_i32]),
    'pm_fft2_spectral': (c_i32, [ctypes.POINTER(pm_fft2_desc), c_i32, ctypes.POINTER(c_f64), ctypes.POINTER(c_f64), c_vp, c_vp, c_vp, c_sz,
                         c_vp]),
    'pm_fft2_mul_ifft2_workspace': (c_sz, [ctypes.POINTER(pm_fft2_desc)]),
    'pm_fft2_mul_ifft2': (c_i32, [ctypes.POINTER(pm_fft2_desc), c_vp, c_vp, c_vp, c_sz, c_vp]),
    'pm_fft2_time_passes': (c_i32, [ctypes.POINTER(pm_fft2_desc), c_vp, c_vp, c_vp, c_sz, c_i32,
                                    ctypes.POINTER(c_f64), c_vp]),
    'pm_fft1': (c_i32, [c_i32, c_i32, c_i32, c_i64, ctypes.POINTER(pm_axis), ctypes.POINTER(pm_axis), c_f64,
                        c_vp, c_i64, c_vp, c_i64, c_vp]),
    'pm_fft1_workspace': (c_sz, [c_i32, c_i32, c_i64, c_i64]),
    'pm_fft1_ws': (c_i32, [c_i32, c_i32, c_i32, c_i64, ctypes.POINTER(pm_axis), ctypes.POINTER(pm_axis), c_f64,
                           c_vp, c_i64, c_vp, c_i64, c_vp, c_sz, c_vp]),
    'pm_czt_vectors': (c_i32, [c_i32, c_i64, c_i64, c_i64, c_f64, c_f64, c_vp, c_vp, c_vp, c_vp]),
    'pm_czt_axis': (c_i32, [c_i32, c_i32, c_i64, c_i64, c_i64, c_i64, c_i64, c_i64, c_vp, c_i32, c_vp, c_i32, c_vp, c_i32, c_f64,
                            c_vp, c_i64, c_vp, c_i64, c_vp]),
    'pm_fft1_ramp': (c_i32, [c_i32, c_i32, c_i32, c_i64, c_i64, c_i64, c_i64, c_i64, c_i64, c_vp, c_i32, c_vp, c_i32, c_f64,
                             c_vp, c_i64, c_vp, c_i64, c_vp]),
    'pm_cmul': (c_i32, [c_i32, c_i32, c_i64, c_i64, c_vp, c_i64, c_vp, c_i64, c_vp, c_i64, c_vp]),
    'pm_rmul': (c_i32, [c_i32, c_i64, c_i64, c_vp, c_i64, c_vp, c_i64, c_f64, c_vp, c_i64, c_vp]),
    'pm_scale_sep': (c_i32, [c_i32, c_i64, c_i64, c_vp, c_i64, c_vp, c_i32, c_vp, c_i32, c_f64, c_vp, c_i64, c_vp]),
    'pm_abs2': (c_i32, [c_i32, c_i64, c_i64, c_vp, c_i64, c_vp, c_i64, c_i32, c_f64, c_vp]),
    'pm_abs_arg': (c_i32, [c_i32, c_i64, c_i64, c_vp, c_i64, c_vp, c_i64, c_vp, c_i64, c_vp]),
    'pm_sum_modes': (c_i32, [c_i32, c_i64, c_i64, c_i64, c_vp, c_i64, c_i64, ctypes.POINTER(c_f64), c_i32, c_vp, c_i64, c_vp]),
    'pm_encircled_energy_workspace': (c_sz, []),
    'pm_encircled_energy': (c_i32, [c_i32, c_i64, c_i64, c_vp, c_i64, c_f64, c_i64, ctypes.POINTER(c_f64), c_vp, c_vp, c_sz, c_vp]),
    'pm_encircled_energy_adjoint': (c_i32, [c_i32, c_i64, c_i64, c_f64, c_i64, ctypes.POINTER(c_f64), ctypes.POINTER(c_f64), c_vp,
                                            c_i64, c_vp]),
    'pm_sample_map': (c_i32, [c_i32, c_i32, c_i64, c_i64, c_vp, c_i64, c_f64, c_f64, c_f64, c_i64, c_i64, c_vp, c_i64, c_i64,
                              c_vp, c_i64, c_i64, c_vp, c_i64, c_f64, c_f64, c_vp, c_i64, c_vp]),
    'pm_spline_prefilter': (c_i32, [c_i32, c_i32, c_i64, c_i64, c_vp, c_i64, c_vp, c_i64, c_vp]),
    'pm_sample_spline': (c_i32, [c_i32, c_i32, c_i64, c_i64, c_vp, c_i64, c_f64, c_f64, c_f64, c_i64, c_i64, c_vp, c_i64, c_i64,
                                 c_vp, c_i64, c_i64, c_vp, c_i64, c_f64, c_f64, c_vp, c_i64, c_vp]),
    'pm_lattice': (c_i32, [c_i32, c_i32, c_i64, c_i64, c_i64, c_i64, c_i64, c_i64, c_i64, c_i64, c_i64, c_f64, c_vp, c_i64, c_i64, c_vp,
                           c_i64, c_i64, c_vp]),
    'pm_warp_workspace': (c_sz, [c_i32, c_i64, c_i64, c_i64]),
    'pm_warp': (c_i32, [c_i32, c_i32, c_i64, c_i64, c_i64, c_vp, c_i64, c_i64, ctypes.POINTER(c_f64), c_f64, c_i64, c_i64, c_i64, c_i64,
                        c_vp, c_i64, c_i64, c_vp, c_sz, c_vp]),
    'pm_zernike_basis': (c_i32, [c_i32, c_i32, c_i64, c_vp, c_vp, c_vp, c_i64, c_i64, c_vp, c_vp]),
    'pm_zernike_sum': (c_i32, [c_i32, c_i32, c_i64, c_vp, c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_i32, c_vp, c_vp]),
    'pm_zernike_project_workspace': (c_sz, [c_i32, c_i64, c_i64, c_i64]),
    'pm_zernike_project': (c_i32, [c_i32, c_i32, c_i64, c_vp, c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_sz, c_vp]),
    'pm_modes_dot_workspace': (c_sz, [c_i32, c_i64, c_i64]),
    'pm_modes_dot': (c_i32, [c_i32, c_i64, c_i64, c_vp, c_i64, c_vp, c_vp, c_vp, c_sz, c_vp]),
    'pm_qpoly_basis': (c_i32, [c_i32, c_i32, c_i64, c_vp, c_vp, c_vp, c_i64, c_i64, c_vp, c_vp]),
    'pm_qpoly_sum': (c_i32, [c_i32, c_i32, c_i64, c_vp, c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_i32, c_vp, c_vp]),
    'pm_qpoly_project_workspace': (c_sz, [c_i32, c_i64, c_i64, c_i64]),
    'pm_qpoly_project': (c_i32, [c_i32, c_i32, c_i64, c_vp, c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_sz, c_vp]),
    'pm_recur_basis': (c_i32, [c_i32, c_i32, c_i64, c_vp, c_vp, c_f64, c_vp, c_i64, c_i64, c_vp, c_vp, c_vp]),
    'pm_recur_sum': (c_i32, [c_i32, c_i32, c_i64, c_vp, c_vp, c_f64, c_vp, c_i64, c_i64, c_i64, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp]),
    'pm_recur_project_workspace': (c_sz, [c_i32, c_i64, c_i64, c_i64]),
    'pm_recur_project': (c_i32, [c_i32, c_i32, c_i64, c_vp, c_vp, c_f64, c_vp, c_i64, c_i64, c_i64, c_i32, c_vp, c_vp, c_i32, c_vp, c_vp, c_sz,
                                 c_vp]),
    'pm_recur2_sum': (c_i32, [c_i32, c_i64, c_i64, c_vp, c_vp, c_vp, c_i64, c_vp, c_i64, c_i64, c_vp, c_i32, c_f64, c_f64, c_vp, c_vp, c_vp,
                              c_i64, c_i64, c_vp]),
    'pm_recur2_project_workspace': (c_sz, [c_i32, c_i64, c_i64, c_i64, c_i64]),
    'pm_recur2_project': (c_i32, [c_i32, c_i64, c_i64, c_vp, c_vp, c_vp, c_i64, c_vp, c_i64, c_i64, c_i32, c_f64, c_f64, c_vp, c_i64, c_i64,
                                  c_i32, c_vp, c_vp, c_sz, c_vp]),
    'pm_recur2_outer': (c_i32, [c_i32, c_i64, c_i64, c_i64, c_vp, c_i64, c_vp, c_i64, c_vp, c_vp, c_vp]),
    'pm_xy_grid': (c_i32, [c_i32, c_i64, c_i64, c_f64, c_i32, c_vp, c_vp, c_vp]),
    'pm_cart_to_polar': (c_i32, [c_i32, c_i64, c_i64, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp]),
    'pm_polar_to_cart': (c_i32, [c_i32, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp]),
    'pm_sdf_render': (c_i32, [c_i32, c_i32, c_i64, c_i64, c_vp, c_vp, c_i64, c_i64, c_f64, c_f64, c_vp, c_i64, c_i64, c_i32, c_f64, c_vp,
                              c_i64, c_i64, c_vp]),
    'pm_bindown': (c_i32, [c_i32, c_i64, c_i64, c_i64, c_i64, c_i64, c_i32, c_vp, c_i64, c_i64, c_vp, c_i64, c_i64, c_vp]),
    'pm_tile': (c_i32, [c_i32, c_i64, c_i64, c_i64, c_i64, c_i64, c_f64, c_vp, c_i64, c_i64, c_vp, c_i64, c_i64, c_vp]),
    'pm_detector_digitize': (c_i32, [c_i32, c_i64, c_i64, c_i64, c_vp, c_i64, c_i64, c_f64, c_f64, c_f64, c_i32, c_vp, c_i64, c_i32, c_vp,
                                     c_vp]),
    'pm_detector_expose': (c_i32, [c_i32, c_i64, c_i64, c_i64, c_vp, c_i64, c_i64, c_vp, c_vp, c_f64, c_f64, c_f64, c_f64, c_f64, c_f64, c_i32,
                                   c_vp, c_i64, c_i32, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp]),
    'pm_detector_words': (c_i32, [c_i64, c_i64, c_i64, c_i64, c_i32, c_vp, c_vp]),
    'pm_bayer_demosaic': (c_i32, [c_i32, c_i32, c_i32, c_i32, c_i64, c_i64, c_i64, c_vp, c_i64, c_i64, c_vp, c_vp]),
    'pm_bayer_weave': (c_i32, [c_i32, c_i32, c_i32, c_i64, c_i64, c_i64] + [c_vp, c_i64, c_i64, c_i64] * 4 + [c_vp, c_i64, c_i64, c_vp]),
    'pm_bayer_deinterlace': (c_i32, [c_i32, c_i32, c_i64, c_i64, c_i64, c_vp, c_i64, c_i64, c_vp, c_vp]),
    'pm_bayer_assemble': (c_i32, [c_i32, c_i64, c_i64, c_i64] + [c_vp, c_i64, c_i64, c_i64] * 4 + [c_vp, c_vp]),
    'pm_bayer_class_max_workspace': (c_sz, []),
    'pm_bayer_class_max': (c_i32, [c_i32, c_i32, c_i64, c_i64, c_i64, c_vp, c_i64, c_i64, c_vp, c_vp, c_sz, c_vp]),
    'pm_bayer_scale': (c_i32, [c_i32, c_i32, c_i32, c_i64, c_i64, c_i64, c_vp, c_i64, c_i64, ctypes.POINTER(c_f64), c_i32, ctypes.POINTER(c_f64),
                               c_vp, c_vp]),
    'pm_optym_cost_workspace': (c_sz, []),
    'pm_optym_cost': (c_i32, [c_i32, c_i32, c_i64, c_vp, c_vp, c_f64, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp]),
    'pm_optym_advance': (c_i32, [c_i32, c_f64, c_f64, c_vp, c_vp, c_vp]),
    'pm_optym_step': (c_i32, [c_i32, c_i32, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_f64, c_f64, c_f64, c_f64, c_vp, c_vp, c_vp, c_vp, c_vp]),
    'pm_optym_activation': (c_i32, [c_i32, c_i32, c_i32, c_i64, c_vp, c_f64, c_f64, c_f64, c_vp, c_vp]),
    'pm_optym_softmax': (c_i32, [c_i32, c_i64, c_i64, c_vp, c_vp, c_f64, c_f64, c_vp, c_vp]),
    'pm_optym_softmax_backprop': (c_i32, [c_i32, c_i64, c_i64, c_vp, c_vp, c_f64, c_vp, c_vp]),
    'pm_optym_spatial_gradient': (c_i32, [c_i32, c_i32, c_i64, c_i64, c_vp, c_vp, c_vp]),
    'pm_lbfgsb_workspace': (c_sz, []),
    'pm_lbfgsb_state_doubles': (c_sz, [c_i32]),
    'pm_lbfgsb_small': (c_i32, [c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    'pm_lbfgsb_dots': (c_i32, [c_i32, c_i64, c_vp, c_vp, c_i64, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp]),
    'pm_lbfgsb_breakpoints': (c_i32, [c_i32, c_i64, c_vp, c_vp, c_i64, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp]),
    'pm_lbfgsb_update': (c_i32, [c_i32, c_i64, c_vp, c_vp, c_i64, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_f64, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp]),
    'pm_lbfgsb_gram': (c_i32, [c_i32, c_i64, c_vp, c_vp, c_i64, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_sz, c_vp]),
    'pm_lbfgsb_combine': (c_i32, [c_i32, c_i32, c_i64, c_vp, c_vp, c_i64, c_i32, c_i32, c_i32, c_f64, c_vp, c_f64, c_vp, c_vp, c_vp, c_vp, c_vp,
                                  c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp]),
    'pm_lbfgsb_cauchy_point': (c_i32, [c_i32, c_i64, c_vp, c_vp, c_vp, c_f64, c_f64, c_vp, c_vp, c_vp]),
    'pm_lbfgsb_trial': (c_i32, [c_i32, c_i64, c_vp, c_vp, c_f64, c_vp, c_vp, c_vp, c_vp]),
    'pm_tf_stack': (c_i32, [c_i32, c_i32, c_i32, c_i64, c_i64, c_vp, c_i64, c_vp, c_i64, c_vp, c_i64, c_i64, c_vp, c_i64, c_i64, c_vp, c_i64, c_vp, c_i64,
                    c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    'pm_tf_thickness_grad_workspace': (c_sz, [c_i32, c_i32, c_i64, c_i64]),
    'pm_tf_thickness_grad': (c_i32, [c_i32, c_i32, c_i64, c_i64, c_vp, c_i64, c_vp, c_i64, c_vp, c_i64, c_i64, c_vp, c_i64, c_i64, c_vp, c_i64, c_vp, c_i64,
                             c_vp, c_vp, c_i64, c_i32, c_vp, c_vp, c_sz, c_vp]),
    'pm_rt_trace': (c_i32, [c_i32, c_i64, c_i64, c_vp, c_f64, c_f64, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    'pm_fiber_modes': (c_i32, [c_i32, c_i64, c_vp, c_vp, c_f64, c_vp, c_i64, c_i64, c_vp, c_vp]),
    'pm_fiber_sum': (c_i32, [c_i32, c_i64, c_vp, c_vp, c_f64, c_vp, c_i64, c_i64, c_i64, c_vp, c_i32, c_vp, c_vp]),
    'pm_fiber_project_workspace': (c_sz, [c_i32, c_i64, c_i64, c_i64]),
    'pm_fiber_project': (c_i32, [c_i32, c_i64, c_vp, c_vp, c_f64, c_vp, c_i64, c_i64, c_i64, c_vp, c_vp, c_vp, c_sz, c_vp]),
    'pm_overlap_workspace': (c_sz, [c_i32, c_i64]),
    'pm_overlap': (c_i32, [c_i32, c_i64, c_vp, c_i32, c_vp, c_i32, c_vp, c_vp, c_sz, c_vp]),
    'pm_object_render': (c_i32, [c_i32, c_i32, c_i32, c_i64, c_i64, c_vp, c_i64, c_vp, c_i64, c_f64, ctypes.POINTER(pm_object), c_vp, c_i64, c_vp]),
    'pm_tf_product': (c_i32, [c_i32, c_i64, c_i64, ctypes.POINTER(pm_tf_freq), ctypes.POINTER(pm_tf_record), c_i64, c_i32, c_vp, c_i64, c_vp]),
    'pm_polar_resample': (c_i32, [c_i32, c_i64, c_i64, c_vp, c_vp, c_f64, c_f64, c_vp, c_vp, c_vp, c_i64, c_vp, c_i64, c_vp]),
    'pm_centroid_workspace': (c_sz, [c_i64, c_i64]),
    'pm_centroid': (c_i32, [c_i32, c_i64, c_i64, c_vp, c_i64, c_vp, c_vp, c_sz, c_vp]),
    'pm_psf_size_workspace': (c_sz, [c_i64]),
    'pm_psf_size_groups': (c_i64, [c_i64]),
    'pm_psf_size': (c_i32, [c_i32, c_i64, c_i64, c_vp, c_i64, c_vp, c_i32, c_f64, c_i32, c_vp, c_vp, c_sz, c_vp]),
    'pm_psi': (c_i32, [c_i32, c_i32, c_i64, c_i64, c_i64, ctypes.POINTER(pm_psi_frames), c_i64, c_vp, c_vp, c_vp, c_i64, c_vp]),
    'pm_lenslet_screen': (c_i32, [c_i32, c_i32, c_i64, c_i64, c_vp, c_i64, c_vp, c_i64, c_f64, ctypes.POINTER(pm_lenslets), c_vp, c_i64, c_vp]),
    'pm_grating': (c_i32, [c_i32, c_i32, c_i32, c_i64, c_i64, c_vp, c_i64, c_f64, c_f64, ctypes.POINTER(c_f64), c_vp, c_i64, c_vp, c_i64, c_vp]),
    'pm_beam_combine': (c_i32, [c_i32, c_i64, c_i64, c_vp, c_i64, c_f64, c_vp, c_i64, c_f64, c_vp, c_i64, c_vp, c_i64, c_vp]),
    'pm_fiber_scale': (c_i32, [c_i32, c_i64, c_i64, c_vp, c_i64, c_vp, c_vp, c_f64, c_f64, c_vp, c_i64, c_vp]),
    'pm_ifg_stats_workspace': (c_sz, [c_i64, c_i64]),
    'pm_ifg_stats': (c_i32, [c_i32, c_i64, c_i64, c_vp, c_i64, c_vp, c_vp, c_sz, c_vp]),
    'pm_ifg_fit_workspace': (c_sz, [c_i64, c_i64]),
    'pm_ifg_fit': (c_i32, [c_i32, c_i32, c_i64, c_i64, c_vp, c_i64, ctypes.POINTER(pm_ifg_coords), c_vp, c_vp, c_sz, c_vp]),
    'pm_ifg_remove': (c_i32, [c_i32, c_i32, c_i64, c_i64, c_vp, c_i64, ctypes.POINTER(pm_ifg_coords), c_vp, c_vp]),
    'pm_ifg_edit': (c_i32, [c_i32, c_i32, c_i64, c_i64, c_vp, c_i64, c_f64, c_vp, c_i64, c_vp, c_vp]),
    'pm_ifg_slope': (c_i32, [c_i32, c_i64, c_i64, c_vp, c_i64, c_f64, c_vp, c_vp, c_vp, c_i64, c_vp]),
    'pm_ifg_window_workspace': (c_sz, [c_i64, c_i64]),
    'pm_ifg_window': (c_i32, [c_i32, c_i32, c_i64, c_i64, c_vp, c_i64, c_f64, c_f64, c_vp, c_i64, c_vp, c_i64, c_vp, c_vp, c_sz, c_vp]),
    'pm_ifg_psd_scale': (c_i32, [c_i32, c_i64, c_i64, c_vp, c_i64, c_vp, c_f64, c_vp]),
    'pm_ifg_band_workspace': (c_sz, [c_i64, c_i64]),
    'pm_ifg_band': (c_i32, [c_i32, c_i32, c_i32, c_i64, c_i64, c_vp, c_i64, c_vp, c_i64, c_f64, c_f64, c_f64, c_vp, c_vp, c_sz, c_vp]),
    'pm_ifg_iir': (c_i32, [c_i32, c_i32, c_i32, c_i64, c_i64, c_vp, c_i64, c_i64, c_i64, c_f64, c_f64, c_f64, c_f64, c_vp, c_vp, c_i64, c_vp]),
    'pm_ifg_combine': (c_i32, [c_i32, c_i32, c_i32, c_i64, c_i64, c_vp, c_i64, c_vp, c_i64, c_vp, c_i64, c_vp]),
    'pm_ifg_psd_model': (c_i32, [c_i32, c_i32, c_i64, c_vp, c_f64, c_f64, c_f64, c_vp, c_vp]),
    'pm_psd_uniform': (c_i32, [c_i32, c_i64, c_i64, c_i64, c_i64, c_i64, c_vp, c_i64, c_i64, c_vp]),
    'pm_psd_signal': (c_i32, [c_i32, c_i64, c_i64, c_i64, c_vp, c_i64, c_i64, c_vp, c_i64, ctypes.POINTER(pm_psd_model), c_f64, c_vp]),
    'pm_psd_finish_workspace': (c_sz, [c_i64, c_i64, c_i64]),
    'pm_psd_finish': (c_i32, [c_i32, c_i32, c_i64, c_i64, c_i64, c_vp, c_i64, c_i64, c_vp, c_i64, c_f64, c_f64, c_vp, c_i64, c_i64, c_vp, c_vp, c_sz, c_vp]),
    'pm_psd_scale': (c_i32, [c_i32, c_i64, c_i64, c_i64, c_vp, c_i64, c_i64, c_vp, c_f64, c_vp]),
    'pm_jones_optic': (c_i32, [c_i32, ctypes.POINTER(pm_jones_optic_desc), c_i64, c_i64, c_vp, c_i64, c_vp, c_i32, c_i64, c_i64, c_vp]),
    'pm_jones_chain': (c_i32, [c_i32, c_i32, ctypes.POINTER(pm_jones_operand), c_i32, c_i32, c_i64, c_i64, c_vp, c_i32, c_i64, c_i64, c_vp]),
    'pm_jones_scale': (c_i32, [c_i32, c_i32, c_i64, c_i64, c_vp, c_i32, c_i64, c_i64, c_i32, c_vp, c_i64, c_vp, c_i32, c_i64, c_i64, c_vp]),
    'pm_jones_to_mueller': (c_i32, [c_i32, c_i64, c_i64, c_vp, c_i32, c_i64, c_i64, c_vp, c_i32, c_i64, c_i64, c_vp]),
    'pm_pauli_coefficients': (c_i32, [c_i32, c_i64, c_i64, c_vp, c_i32, c_i64, c_i64, c_vp, c_i64, c_i64, c_vp]),
    'pm_modes_record_doubles': (c_sz, [c_i64, c_i64]),
    'pm_modes_gram_workspace': (c_sz, [c_i32, c_i64, c_i64, c_i64]),
    'pm_modes_gram': (c_i32, [c_i32, c_i32, c_i64, c_i64, c_vp, c_i64, c_i64, c_vp, c_i64, c_vp, c_i32, c_vp, c_vp, c_sz, c_vp]),
    'pm_modes_small': (c_i32, [c_i32, c_i32, c_i64, c_i64, c_vp, c_vp, c_vp, c_vp]),
    'pm_modes_transform': (c_i32, [c_i32, c_i32, c_i32, c_i64, c_i64, c_vp, c_i64, c_vp, c_vp, c_vp, c_i64, c_vp]),
    'pm_modes_stats_workspace': (c_sz, [c_i64, c_i64]),
    'pm_modes_stats': (c_i32, [c_i32, c_i64, c_i64, c_vp, c_i64, c_vp, c_vp, c_vp, c_sz, c_vp]),
    'pm_segment_plan_check': (c_i32, [c_i64, c_i64, c_i64, c_vp, c_i64, c_i64, c_i64]),
    'pm_segment_compose': (c_i32, [c_i32, c_i32, c_i64, c_i64, c_vp, c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, c_vp, c_i64, c_i64, c_vp, c_i64,
                                   c_vp, c_i32, c_vp, c_vp]),
    'pm_segment_project_workspace': (c_sz, [c_i32, c_i64, c_i64, c_i64, c_i64]),
    'pm_segment_project': (c_i32, [c_i32, c_i32, c_i64, c_i64, c_vp, c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, c_i64, c_i64, c_vp, c_i64,
                                   c_vp, c_vp, c_vp, c_sz, c_vp]),
    'pm_pupil_synth': (c_i32, [c_i32, c_i64, c_i64, c_vp, c_i32, c_i64, c_vp, c_i64, c_f64, c_vp, c_i64, c_vp]),
    'pm_quadratic_phase': (c_i32, [c_i32, c_i64, c_i64, c_vp, c_i64, c_vp, c_i64, c_f64, c_vp, c_i64, c_vp]),
    'pm_as_tf_vectors': (c_i32, [c_i32, c_i64, c_i64, c_f64, c_f64, c_f64, c_vp, c_vp, c_vp]),
    'pm_outer': (c_i32, [c_i32, c_i64, c_i64, c_vp, c_vp, c_vp, c_i64, c_vp]),
    'pm_embed': (c_i32, [c_i32, c_i64, c_i64, c_vp, c_i64, c_i64, c_i64, c_i64, c_i64, c_vp, c_vp, c_i64, c_vp]),
    'pm_pad_index': (c_i32, [c_i32, c_i32, c_i64, c_i64, c_vp, c_i64, c_i64, c_i64, c_i64, c_i64, c_vp, c_i64, c_vp]),
    'pm_mdft_basis': (c_i32, [c_i32, c_i64, c_i64, c_vp, c_vp, c_i32, c_vp, c_i64, c_vp]),
    'pm_mdft_basis_grid': (c_i32, [c_i32, c_i64, c_i64, c_f64, c_f64, c_f64, c_f64, c_i32, c_vp, c_i64, c_vp]),
    'pm_cgemm': (c_i32, [c_i32, c_i32, c_i32, c_i64, c_i64, c_i64, c_f64, c_vp, c_i64, c_vp, c_i64, c_vp, c_i64,
                         c_vp, c_sz, c_vp]),
    'pm_cgemm_workspace': (c_sz, [c_i32, c_i64, c_i64, c_i64]),
    'pm_cgemm_abs2': (c_i32, [c_i32, c_i32, c_i32, c_i64, c_i64, c_i64, c_f64, c_vp, c_i64, c_vp, c_i64, c_vp, c_i64, c_f64, c_i32,
                              c_vp, c_sz, c_vp]),
}

_lib = None


def load():
    """Load libprysm_amd.so; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f'{LIB_PATH} is missing: build it with `make -C prysm_amd/csrc -j8` (or '
            '`python -c "import __graft_entry__ as g; g.build()"`).  prysm_amd has no CPU fallback.')
    lib = ctypes.CDLL(LIB_PATH)
    other_build = bool(os.environ.get('PRYSM_AMD_LIB'))
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)   # AttributeError here = the library does not export a declared symbol
        except AttributeError:
            if other_build:           # an OLDER build under test (tools/exp_ab_libs.py): it may predate an entry point; calling it raises
                continue
            raise
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


class PrysmAmdError(RuntimeError):
    """A HIP runtime error reported by libprysm_amd.so."""


def check(rc):
    """Translate a C return code into the exception class the reference would raise."""
    if rc == 0:
        return
    lib = load()
    if rc < 0:
        msg = lib.pm_last_error().decode(errors='replace')
        if rc == PM_ERR_UNSUPPORTED:
            raise NotImplementedError(msg)
        raise ValueError(msg)
    raise PrysmAmdError(f'libprysm_amd: HIP error {rc} (hipError_t); is an MI355X visible?')


# --------------------------------------------------------------------------- tensors

_COMPLEX_CODE = {torch.complex64: PM_C64, torch.complex128: PM_C128}
_REAL_OF = {torch.complex64: torch.float32, torch.complex128: torch.float64}
_COMPLEX_OF = {torch.float32: torch.complex64, torch.float64: torch.complex128, torch.float16: torch.complex64}
_NP2TORCH = {
    np.dtype('float32'): torch.float32, np.dtype('float64'): torch.float64, np.dtype('float16'): torch.float16,
    np.dtype('complex64'): torch.complex64, np.dtype('complex128'): torch.complex128, np.dtype('bool'): torch.bool,
    np.dtype('int32'): torch.int32, np.dtype('int64'): torch.int64, np.dtype('uint8'): torch.uint8,
    np.dtype('uint16'): torch.uint16, np.dtype('uint32'): torch.uint32, np.dtype('uint64'): torch.uint64, np.dtype('int16'): torch.int16,
    np.dtype('int8'): torch.int8,
}


_have_gpu = None
_devices = {}


def device():
    """The MI355X this process computes on (torch's current device)."""
    global _have_gpu
    if _have_gpu is None:
        _have_gpu = torch.cuda.is_available()       # asked once: the answer does not change within a process, the question costs 2 us
        if _have_gpu:
            torch.cuda.init()      # the raw accessors below assume torch's lazy runtime initialisation has happened
    if not _have_gpu:
        raise RuntimeError('prysm_amd needs an AMD MI355X (gfx950) visible to PyTorch-ROCm; there is no CPU path')
    i = _cur_dev()
    d = _devices.get(i)
    if d is None:
        d = _devices[i] = torch.device('cuda', i)
    return d


# torch.cuda.current_stream() / current_device() build Python objects and re-check the runtime on every call (~6 us of the ~21 us a
# small propagation costs on the host, experiments/scripts/exp_host_profile.py); the raw accessors return the same integers
_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)
_raw_device = getattr(torch._C, '_cuda_getDevice', None)


def _cur_dev():
    return _raw_device() if _raw_device is not None else torch.cuda.current_device()


def _cur_stream():
    """hipStream_t of torch's current stream on the current device, as an integer."""
    if _raw_stream is not None:
        return _raw_stream(_cur_dev())
    return torch.cuda.current_stream().cuda_stream


def torch_dtype(dt):
    """numpy dtype-like or torch dtype -> torch dtype."""
    if isinstance(dt, torch.dtype):
        return dt
    return _NP2TORCH[np.dtype(dt)]


def as_device(x, dtype=None):
    """numpy array / torch tensor / scalar sequence -> contiguous tensor in HBM."""
    dev = device()
    if isinstance(x, torch.Tensor):
        t = x.to(dev) if x.device != dev else x
    else:
        a = np.ascontiguousarray(x)
        t = torch.from_numpy(a).to(dev)
    if dtype is not None and t.dtype != dtype:
        t = t.to(dtype)
    if t.is_conj() or t.is_neg():       # torch's lazy conj / neg views: the library reads the stored bytes
        t = t.resolve_conj().resolve_neg()
    if not t.is_contiguous():
        t = t.contiguous()
    return t


def as_complex(x, at_least=None):
    """Promote like numpy does for fft input: f32 -> c64, everything else real -> c128; keep complex.

    `at_least` (a torch complex dtype) raises c64 to c128 when config.precision demands it.
    """
    t = as_device(x)
    if not t.is_complex():
        t = t.to(_COMPLEX_OF.get(t.dtype, torch.complex128))
    if at_least is not None and at_least == torch.complex128 and t.dtype == torch.complex64:
        t = t.to(torch.complex128)
    return t


def as_field(x):
    """Like as_complex, but float32 / float64 arrays stay REAL: the 2-D transforms read them directly
    (PM_FLAG_REAL_INPUT), which halves the bytes of the first pass and avoids a complex copy."""
    t = as_device(x)
    if t.is_complex() or t.dtype in (torch.float32, torch.float64):
        return t
    return as_complex(t)


def cdtype_of(t):
    """Complex dtype a transform of `t` produces."""
    return t.dtype if t.is_complex() else _COMPLEX_OF[t.dtype]


def code(t):
    return _COMPLEX_CODE[cdtype_of(t)]


def stream_ptr():
    return ctypes.c_void_p(_cur_stream())


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


class tuning_local:
    """``with tuning_local(fold=0, mix=0): ...`` -- performance knobs for the CALLING THREAD only (pm_set_tuning_local), restored on
    exit.  The process-wide pm_set_tuning is for start-up configuration; two threads driving the library at once (one pipeline per
    thread, prysm's own advice) each take this.

    Blocks nest: the library keeps ONE private copy of the knobs per thread and can only reset it as a whole, so this class keeps the
    thread's stack of open blocks and re-applies the outer ones when an inner block ends (or fails to start -- a knob the build
    refuses leaves nothing half-applied).  Knobs set by direct pm_set_tuning_local calls are outside that stack and are lost at the
    first exit."""

    _tls = threading.local()
    epoch = 0       # bumped whenever a block starts or ends: answers derived from the planner (e.g. _ops.on_register_engine) are cached per epoch

    def __init__(self, **knobs):
        self.knobs = knobs

    @classmethod
    def signature(cls):
        """the calling thread's open blocks as a hashable value: what a cached planner answer is valid for"""
        return tuple(tuple(sorted(b.items())) for b in getattr(cls._tls, 'stack', ()))

    @classmethod
    def _replay(cls, lib):
        lib.pm_reset_tuning_local()
        for outer in getattr(cls._tls, 'stack', []):
            for k, v in outer.items():
                lib.pm_set_tuning_local(k.encode(), int(v))

    def __enter__(self):
        lib = load()
        try:
            for k, v in self.knobs.items():
                check(lib.pm_set_tuning_local(k.encode(), int(v)))
        except Exception:
            self._replay(lib)
            raise
        if not hasattr(self._tls, 'stack'):
            self._tls.stack = []
        self._tls.stack.append(dict(self.knobs))
        tuning_local.epoch += 1
        return self

    def __exit__(self, *exc):
        stack = getattr(self._tls, 'stack', [])
        if stack:
            stack.pop()
        self._replay(load())
        tuning_local.epoch += 1
        return False


_workspaces = {}


def workspace(nbytes):
    """Scratch buffer in HBM, reused per (device, stream); stream-ordered so back-to-back calls are safe."""
    if nbytes <= 0:
        return None
    key = (_cur_dev(), _cur_stream())
    w = _workspaces.get(key)
    if w is None or w.numel() < nbytes:
        w = torch.empty(int(nbytes), dtype=torch.uint8, device=device())
        _workspaces[key] = w
    return w
