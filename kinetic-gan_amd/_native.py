"""ctypes binding of libkgan_hip.so (C ABI in include/kgan_hip.h) for torch tensors.

Every function here takes torch CUDA tensors, borrows their device pointers, enqueues HIP kernels
on torch's current stream and returns torch tensors allocated by torch's caching allocator.  There
is deliberately NO fallback: if the library is missing or a tensor is not on the GPU the call
raises.  (tests/ swap these functions for torch emulations to exercise the autograd composition
on a CPU-only box; the product never does.)

"Plane tensor" = logical (N, C, T, V) tensor whose (t, v) plane is contiguous; see kgan_hip.h.

How an entry point is bound - the idioms are written once:
  * ``_Foo`` mirrors the header's ``KgFoo`` field for field, ``X`` its ``#define KG_X`` (tests/test_abi_cpu.py compares every
    size, offset and constant with the compiled header).
  * ``_bind(a, field, prefix, t)`` writes a plane operand (pointer, <prefix>_sN, <prefix>_sC); ``_plane(t)`` makes the
    KgPlane-typed fields of the fused generator block.  Special addressing (a broadcast operand, an offset output) is
    spelled out where it happens.
  * ``_query`` asks a ``*_bytes`` size query and raises the library's message when it answers < 0; ``_workspace`` also
    allocates the scratch and attaches it (and the ticket counters of ``_sync_buffer``) to the struct, or hands it to a
    ``*_many`` launcher's (ws, bytes) arguments.
  * A struct that a single and a ``_many`` entry point share has ONE filler (``_conv_args``, ``_wgrad_args``,
    ``_rowsum_fill``, ``_bn_fwd_fill``, ``_bn_bwd_fill``, ``_gp_args``, ``_head_args``); the ``_many`` form loops over it.
  * ``_dest`` checks a flat fp32 destination, ``_chunks`` walks a job table in launches of at most X_MAX_JOBS entries.
  * Lifetime: a tensor whose pointer sits in a struct must stay referenced until the launch call has returned (stream order
    protects it afterwards).  ``as_plane`` / ``contiguous`` copies and scratch tensors have no other owner, so the helpers
    RETURN what they bound and the callers hold it (``keep`` / ``held`` / ``ws``) - these names look unused and are not.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import NamedTuple, Optional, Sequence, Tuple

import torch

_PKG = os.path.dirname(os.path.abspath(__file__))
# KG_LIB: an experiment build of the library (tools/build_variant.sh, A/B timing); the default is the in-tree build
LIB_PATH = os.environ.get("KG_LIB") or os.path.join(_PKG, "libkgan_hip.so")

ACT_NONE, ACT_LRELU, ACT_TANH = 0, 1, 2
ABI_VERSION = 9
TAP_TIME, TAP_CHANBLOCK = 0, 1

c_f32p = C.c_void_p
c_i32p = C.c_void_p


class _ConvGroup(C.Structure):
    _fields_ = [("x", c_f32p), ("x_sN", C.c_int64), ("x_sC", C.c_int64),
                ("Cin", C.c_int32), ("T_in", C.c_int32), ("V_in", C.c_int32),
                ("x_lead", C.c_int32),
                ("vmap", c_i32p),
                ("w", c_f32p), ("w_sT", C.c_int64), ("w_sO", C.c_int64), ("w_sI", C.c_int64),
                ("w_sMB", C.c_int64), ("w_MB", C.c_int32),
                ("taps", C.c_int32), ("tap_mode", C.c_int32), ("t_stride", C.c_int32),
                ("transposed", C.c_int32)]


class _ConvArgs(C.Structure):
    _fields_ = [("N", C.c_int32), ("M", C.c_int32), ("T_out", C.c_int32), ("V_out", C.c_int32),
                ("out", c_f32p), ("o_sN", C.c_int64), ("o_sC", C.c_int64),
                ("ngroups", C.c_int32),
                ("g", _ConvGroup * 2),
                ("bias0", c_f32p), ("bias1", c_f32p),
                ("add", c_f32p), ("a_sN", C.c_int64), ("a_sC", C.c_int64), ("a_tstride", C.c_int32),
                ("act", C.c_int32), ("slope", C.c_float),
                ("ws", c_f32p), ("ws_bytes", C.c_int64),
                ("mask", c_f32p), ("m_sN", C.c_int64), ("m_sC", C.c_int64),
                ("sync", C.c_void_p), ("sync_len", C.c_int32),
                ("o_tstride", C.c_int32),
                ("wpack", C.c_void_p), ("wpack_bytes", C.c_int64)]


class _WgradPair(C.Structure):
    _fields_ = [("N", C.c_int32),
                ("g", c_f32p), ("g_sN", C.c_int64), ("g_sC", C.c_int64),
                ("x", c_f32p), ("x_sN", C.c_int64), ("x_sC", C.c_int64)]


class _WgradArgs(C.Structure):
    _fields_ = [("N", C.c_int32), ("M", C.c_int32), ("T_out", C.c_int32), ("V_out", C.c_int32),
                ("g", c_f32p), ("g_sN", C.c_int64), ("g_sC", C.c_int64),
                ("x", c_f32p), ("x_sN", C.c_int64), ("x_sC", C.c_int64),
                ("Cin", C.c_int32), ("T_in", C.c_int32), ("V_in", C.c_int32),
                ("vmap", c_i32p),
                ("taps", C.c_int32), ("tap_mode", C.c_int32), ("t_stride", C.c_int32),
                ("dw", c_f32p), ("w_sT", C.c_int64), ("w_sO", C.c_int64), ("w_sI", C.c_int64),
                ("ws", c_f32p), ("ws_bytes", C.c_int64), ("accumulate", C.c_int32),
                ("nextra", C.c_int32), ("extra", _WgradPair * 2), ("defer_reduce", C.c_int32)]


class _WgradReduceJob(C.Structure):
    _fields_ = [("ws", c_f32p), ("dw", c_f32p), ("w_sT", C.c_int64), ("w_sO", C.c_int64), ("w_sI", C.c_int64),
                ("taps", C.c_int32), ("M", C.c_int32), ("Cin", C.c_int32), ("splits", C.c_int32),
                ("accumulate", C.c_int32)]


WGRAD_REDUCE_MAX_JOBS = 24
# tile variants of the weight-gradient kernels (KG_WGRAD_TILE_* of kgan_hip.h: output rows x input channels per workgroup)
WGRAD_TILE_128x128, WGRAD_TILE_64x64, WGRAD_TILE_64x32, WGRAD_TILE_32x64, WGRAD_TILE_32x32 = 0, 1, 2, 3, 4
WGRAD_TILE_NAMES = {WGRAD_TILE_128x128: "128x128", WGRAD_TILE_64x64: "64x64", WGRAD_TILE_64x32: "64x32",
                    WGRAD_TILE_32x64: "32x64", WGRAD_TILE_32x32: "32x32"}
WGRAD_MAX_SPLITS = 128          # partial slabs of one layer (make_plan's cap; one more per extra operand pair at most)


class _WgradReduceJobs(C.Structure):
    _fields_ = [("njobs", C.c_int32), ("job", _WgradReduceJob * WGRAD_REDUCE_MAX_JOBS)]


class _AggArgs(C.Structure):
    _fields_ = [("N", C.c_int32), ("C", C.c_int32), ("K", C.c_int32), ("V", C.c_int32), ("W", C.c_int32),
                ("T", C.c_int32), ("rep", C.c_int32),
                ("a", c_f32p),
                ("x", c_f32p), ("x_sN", C.c_int64), ("x_sC", C.c_int64),
                ("y", c_f32p), ("y_sN", C.c_int64), ("y_sC", C.c_int64),
                ("out", c_f32p), ("o_sN", C.c_int64), ("o_sC", C.c_int64),
                ("ws", c_f32p), ("ws_bytes", C.c_int64), ("a_transposed", C.c_int32), ("defer_sum", C.c_int32),
                ("res", c_f32p), ("r_sN", C.c_int64), ("r_sC", C.c_int64), ("r_T", C.c_int32), ("r_V", C.c_int32),
                ("r_tstride", C.c_int32), ("r_inv", c_i32p),
                ("mask", c_f32p), ("m_sN", C.c_int64), ("m_sC", C.c_int64), ("slope", C.c_float)]


AGG_OP_EXPAND, AGG_OP_REDUCE, AGG_OP_OUTER = 0, 1, 2
# kernel forms of the aggregation family, as kg_agg_plan_info names them
AGG_FORM_FRAME, AGG_FORM_STREAM, AGG_FORM_MFMA, AGG_FORM_OUTER_ELEM, AGG_FORM_OUTER_MFMA = 0, 1, 2, 3, 4
AGG_FORM_NAMES = {AGG_FORM_FRAME: "frame", AGG_FORM_STREAM: "stream", AGG_FORM_MFMA: "mfma",
                  AGG_FORM_OUTER_ELEM: "outer-elementwise", AGG_FORM_OUTER_MFMA: "outer-mfma"}


class _AggPlanInfo(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "form", "K", "WP", "VM", "FO", "KI", "KO", "KS", "RES", "MSK", "SUB", "tiles_per_c", "ntiles", "TV", "TW",
        "P", "F", "chunks", "units", "slabs", "grid_x", "grid_y", "lds_bytes")]


class _AggConvPlanInfo(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "tiny", "MT", "RG", "LB", "BM", "KS", "XE", "XA", "ADD", "tapmask", "spanp", "grid_x", "grid_y", "lds_bytes")]


# kernel families of kg_conv / kg_conv_many, as kg_conv_form_info names them
CONV_FAMILY_DIRECT, CONV_FAMILY_TINY, CONV_FAMILY_BS, CONV_FAMILY_BSW, CONV_FAMILY_MANY, CONV_FAMILY_RING = 0, 1, 2, 3, 4, 5
CONV_FAMILY_NAMES = {CONV_FAMILY_DIRECT: "direct", CONV_FAMILY_TINY: "tiny", CONV_FAMILY_BS: "bs", CONV_FAMILY_BSW: "bsw",
                     CONV_FAMILY_MANY: "many", CONV_FAMILY_RING: "ring"}


class _ConvFormInfo(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "family", "tile", "BM", "NW", "KW", "KF", "FAST", "PLAIN", "INK", "TM", "RWV", "CWV", "MT", "nsplit", "per",
        "epilogue", "pack", "wpack")] + [("win", C.c_int32 * 2)] + [(n, C.c_int32) for n in ("xcd", "grid_x", "grid_y", "grid_z")]


class _ConvManyForm(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("tile", "BM", "KF", "PLAIN", "njobs", "total_wg")] + [
        ("xcd", C.c_int32 * 4), ("wg_begin", C.c_int32 * 4), ("nwg", C.c_int32 * 4)]


def plan_dict(p) -> dict:
    """a plan report (_AggPlanInfo / _AggConvPlanInfo) as a plain dict"""
    return {n: (getattr(p, n) if isinstance(getattr(p, n), int) else list(getattr(p, n))) for n, _ in p._fields_}


class _OuterSumJob(C.Structure):
    _fields_ = [("ws", c_f32p), ("out", c_f32p), ("nout", C.c_int32), ("slabs", C.c_int32)]


OUTER_SUM_MAX_JOBS = 16


class _OuterSumJobs(C.Structure):
    _fields_ = [("njobs", C.c_int32), ("job", _OuterSumJob * OUTER_SUM_MAX_JOBS)]


class _AggConvArgs(C.Structure):
    _fields_ = [("N", C.c_int32), ("Cin", C.c_int32), ("M", C.c_int32), ("T", C.c_int32), ("V", C.c_int32),
                ("W", C.c_int32), ("K", C.c_int32),
                ("x", c_f32p), ("x_sN", C.c_int64), ("x_sC", C.c_int64),
                ("a", c_f32p), ("a_transposed", C.c_int32),
                ("nbr", c_i32p), ("pcount", C.c_int32 * 3),
                ("w", c_f32p), ("w_sT", C.c_int64), ("w_sO", C.c_int64), ("w_sI", C.c_int64),
                ("out", c_f32p), ("o_sN", C.c_int64), ("o_sC", C.c_int64),
                ("add", c_f32p), ("a_sN", C.c_int64), ("a_sC", C.c_int64), ("a_tstride", C.c_int32),
                ("xa", c_f32p), ("xa_sN", C.c_int64), ("xa_sC", C.c_int64)]


class _RowsumArgs(C.Structure):
    _fields_ = [("N", C.c_int32), ("C", C.c_int32), ("T", C.c_int32), ("V", C.c_int32),
                ("x", c_f32p), ("x_sN", C.c_int64), ("x_sC", C.c_int64),
                ("y", c_f32p), ("y_sN", C.c_int64), ("y_sC", C.c_int64),
                ("shift", c_f32p),
                ("want_second", C.c_int32),
                ("out", c_f32p),
                ("ws", c_f32p), ("ws_bytes", C.c_int64), ("accumulate", C.c_int32), ("out2", c_f32p)]


class _BnArgs(C.Structure):
    _fields_ = [("N", C.c_int32), ("C", C.c_int32), ("T", C.c_int32), ("V", C.c_int32),
                ("x", c_f32p), ("x_sN", C.c_int64), ("x_sC", C.c_int64),
                ("g", c_f32p), ("g_sN", C.c_int64), ("g_sC", C.c_int64),
                ("gamma", c_f32p), ("beta", c_f32p),
                ("running_mean", c_f32p), ("running_var", c_f32p),
                ("num_batches_tracked", C.c_void_p),
                ("mean", c_f32p), ("rstd", c_f32p),
                ("momentum", C.c_float), ("eps", C.c_float),
                ("training", C.c_int32),
                ("coef", c_f32p)]


class _BnJob(C.Structure):
    _fields_ = [("a", _BnArgs), ("groups", C.c_int32)]


class _GpArgs(C.Structure):
    _fields_ = [("N", C.c_int32), ("C", C.c_int32), ("T", C.c_int32), ("V", C.c_int32),
                ("g", c_f32p), ("g_sN", C.c_int64), ("g_sC", C.c_int64),
                ("nrm", c_f32p), ("gp", c_f32p), ("gout", c_f32p),
                ("out", c_f32p), ("o_sN", C.c_int64), ("o_sC", C.c_int64)]


class _EltArgs(C.Structure):
    _fields_ = [("N", C.c_int32), ("C", C.c_int32), ("T", C.c_int32), ("V", C.c_int32),
                ("x", c_f32p), ("x_sN", C.c_int64), ("x_sC", C.c_int64),
                ("r", c_f32p), ("r_sN", C.c_int64), ("r_sC", C.c_int64),
                ("noise", c_f32p),
                ("sx", c_f32p), ("bx", c_f32p), ("sr", c_f32p), ("br", c_f32p), ("nw", c_f32p),
                ("out", c_f32p), ("o_sN", C.c_int64), ("o_sC", C.c_int64),
                ("act", C.c_int32), ("slope", C.c_float),
                ("groups", C.c_int32), ("coef_gs", C.c_int64)]


class _GenArgs(C.Structure):
    _fields_ = [("N", C.c_int32), ("C", C.c_int32), ("K", C.c_int32), ("Cr", C.c_int32), ("Tc", C.c_int32),
                ("Vc", C.c_int32), ("V", C.c_int32), ("rep", C.c_int32),
                ("a", c_f32p), ("u", c_f32p), ("b", c_f32p),
                ("y", c_f32p), ("y_out", c_f32p), ("y_sN", C.c_int64), ("y_sC", C.c_int64),
                ("z", c_f32p), ("z_sN", C.c_int64), ("z_sC", C.c_int64),
                ("zf", c_f32p), ("zf_sN", C.c_int64), ("zf_sC", C.c_int64),
                ("rs", c_f32p), ("rs_out", c_f32p), ("rs_sN", C.c_int64), ("rs_sC", C.c_int64),
                ("rbias", c_f32p),
                ("r", c_f32p), ("r_sN", C.c_int64), ("r_sC", C.c_int64)]


class _GenAdjJob(C.Structure):
    _fields_ = [("dbt", c_f32p), ("u", c_f32p), ("a", c_f32p), ("out", c_f32p),
                ("K", C.c_int32), ("Kd", C.c_int32), ("V", C.c_int32), ("Vc", C.c_int32), ("accumulate", C.c_int32)]


class _HeadArgs(C.Structure):
    _fields_ = [("N", C.c_int32), ("C", C.c_int32), ("T", C.c_int32), ("V", C.c_int32),
                ("h", c_f32p), ("h_sN", C.c_int64), ("h_sC", C.c_int64),
                ("w", c_f32p), ("b", c_f32p), ("v", c_f32p), ("gv", c_f32p),
                ("g", c_f32p), ("g_sN", C.c_int64), ("g_sC", C.c_int64),
                ("slope", C.c_float), ("masked", C.c_int32),
                ("dw", c_f32p), ("db", c_f32p), ("accumulate", C.c_int32)]


class _LinearArgs(C.Structure):
    _fields_ = [("N", C.c_int32), ("Din", C.c_int32), ("Dout", C.c_int32), ("L", C.c_int32), ("J", C.c_int32),
                ("x", c_f32p), ("x_ld", C.c_int64), ("emb", c_f32p), ("labels", C.c_void_p),
                ("w", c_f32p), ("bias", c_f32p), ("y", c_f32p), ("y_ld", C.c_int64),
                ("act", C.c_int32), ("slope", C.c_float),
                ("g", c_f32p), ("g_ld", C.c_int64),
                ("gx", c_f32p), ("gx_ld", C.c_int64), ("gx_cols", C.c_int32),
                ("dw", c_f32p), ("db", c_f32p), ("demb", c_f32p), ("accumulate", C.c_int32)]


class _LabelBiasArgs(C.Structure):
    _fields_ = [("N", C.c_int32), ("L", C.c_int32), ("J", C.c_int32), ("K", C.c_int32), ("C", C.c_int32),
                ("V", C.c_int32), ("W", C.c_int32), ("T", C.c_int32),
                ("labels", C.c_void_p), ("emb", c_f32p),
                ("w", c_f32p), ("w_sK", C.c_int64), ("w_sC", C.c_int64),
                ("ak", c_f32p), ("zl", c_f32p),
                ("gz", c_f32p), ("gz_sN", C.c_int64), ("gz_sC", C.c_int64),
                ("demb", c_f32p), ("dw", c_f32p), ("accumulate", C.c_int32),
                ("dak", c_f32p), ("dak_accumulate", C.c_int32),
                ("ws", c_f32p), ("ws_bytes", C.c_int64)]


class _MixArgs(C.Structure):
    _fields_ = [("N", C.c_int32), ("C", C.c_int32), ("T", C.c_int32), ("V", C.c_int32),
                ("real", c_f32p), ("r_sN", C.c_int64), ("r_sC", C.c_int64),
                ("fake", c_f32p), ("f_sN", C.c_int64), ("f_sC", C.c_int64),
                ("alpha", c_f32p),
                ("out", c_f32p), ("o_sN", C.c_int64), ("o_sC", C.c_int64)]


class _MaskedAdjArgs(C.Structure):
    _fields_ = [("n", C.c_int32), ("a", c_f32p), ("imp", c_f32p), ("sel", C.c_void_p), ("ak", c_f32p),
                ("g", c_f32p), ("dimp", c_f32p), ("accumulate", C.c_int32)]


class _GenTailArgs(C.Structure):
    _fields_ = [("N", C.c_int32), ("C", C.c_int32), ("T", C.c_int32), ("V", C.c_int32), ("act", C.c_int32), ("slope", C.c_float),
                ("g", c_f32p), ("g_sN", C.c_int64), ("g_sC", C.c_int64),
                ("out", c_f32p), ("o_sN", C.c_int64), ("o_sC", C.c_int64),
                ("u", c_f32p), ("u_sN", C.c_int64), ("u_sC", C.c_int64), ("mean_t", c_f32p), ("rstd_t", c_f32p), ("gamma_t", c_f32p),
                ("r", c_f32p), ("r_sN", C.c_int64), ("r_sC", C.c_int64), ("mean_r", c_f32p), ("rstd_r", c_f32p), ("gamma_r", c_f32p),
                ("noise", c_f32p), ("coef", c_f32p),
                ("dgamma_t", c_f32p), ("dbeta_t", c_f32p), ("dgamma_r", c_f32p), ("dbeta_r", c_f32p), ("dnw", c_f32p),
                ("ws", c_f32p), ("ws_bytes", C.c_int64), ("counters", C.c_void_p), ("counters_len", C.c_int32),
                ("du", c_f32p), ("du_sN", C.c_int64), ("du_sC", C.c_int64),
                ("dr", c_f32p), ("dr_sN", C.c_int64), ("dr_sC", C.c_int64)]


class _GenPrepJob(C.Structure):
    _fields_ = [("a", c_f32p), ("imp", c_f32p), ("u", c_f32p), ("aeff", c_f32p), ("b", c_f32p),
                ("K", C.c_int32), ("V", C.c_int32), ("Vc", C.c_int32)]


class _Plane(C.Structure):
    _fields_ = [("p", c_f32p), ("sN", C.c_int64), ("sC", C.c_int64)]


class _GenBnLayer(C.Structure):
    _fields_ = [("gamma", c_f32p), ("beta", c_f32p), ("running_mean", c_f32p), ("running_var", c_f32p),
                ("num_batches_tracked", C.c_void_p), ("momentum", C.c_float), ("eps", C.c_float), ("coef", c_f32p)]


class _GenBlockArgs(C.Structure):
    _fields_ = [("N", C.c_int32), ("groups", C.c_int32),
                ("Cin", C.c_int32), ("C", C.c_int32), ("K", C.c_int32), ("Kp", C.c_int32),
                ("Tc", C.c_int32), ("Vc", C.c_int32), ("T", C.c_int32), ("V", C.c_int32), ("rep", C.c_int32),
                ("res_kind", C.c_int32), ("bn_t", C.c_int32), ("act", C.c_int32), ("slope", C.c_float),
                ("x", _Plane),
                ("pu", _Plane), ("pr", _Plane), ("pcoef_t", c_f32p), ("pcoef_r", c_f32p), ("pnoise", c_f32p), ("pnw", c_f32p),
                ("pact", C.c_int32), ("xout", _Plane),
                ("wg", c_f32p), ("wr", c_f32p), ("br", c_f32p), ("wt", c_f32p), ("bt", c_f32p),
                ("b", c_f32p), ("u", c_f32p),
                ("yc", _Plane), ("z", _Plane), ("r", _Plane), ("uo", _Plane),
                ("bt_", _GenBnLayer), ("br_", _GenBnLayer),
                ("noise", c_f32p), ("nw", c_f32p), ("out", _Plane),
                ("ws", c_f32p), ("ws_bytes", C.c_int64), ("counters", C.c_void_p), ("counters_len", C.c_int32)]


class _GenBlockBwdArgs(C.Structure):
    _fields_ = [("N", C.c_int32),
                ("Cin", C.c_int32), ("C", C.c_int32), ("K", C.c_int32), ("Kp", C.c_int32),
                ("Tc", C.c_int32), ("Vc", C.c_int32), ("T", C.c_int32), ("V", C.c_int32), ("rep", C.c_int32),
                ("res_kind", C.c_int32), ("bn_t", C.c_int32), ("act", C.c_int32), ("slope", C.c_float),
                ("g", _Plane), ("out", _Plane), ("uo", _Plane), ("r", _Plane),
                ("coef", c_f32p),
                ("wg", c_f32p), ("wr", c_f32p), ("wt", c_f32p), ("b", c_f32p), ("u", c_f32p),
                ("du", _Plane), ("dr", _Plane), ("gyc", _Plane), ("zf", _Plane), ("gx", _Plane),
                ("px", _Plane), ("pu", _Plane), ("pr", _Plane), ("pnoise", c_f32p), ("pact", C.c_int32),
                ("pmean_t", c_f32p), ("prstd_t", c_f32p), ("pgamma_t", c_f32p),
                ("pmean_r", c_f32p), ("prstd_r", c_f32p), ("pgamma_r", c_f32p),
                ("pcoef", c_f32p), ("dgamma_t", c_f32p), ("dbeta_t", c_f32p), ("dgamma_r", c_f32p), ("dbeta_r", c_f32p),
                ("dnw", c_f32p),
                ("ws", c_f32p), ("ws_bytes", C.c_int64), ("counters", C.c_void_p), ("counters_len", C.c_int32)]


GB_DIR_FWD, GB_DIR_BWD, GB_DIR_INFER = 0, 1, 2       # KgGenBlockFormQuery.dir


class _GenBlockFormQuery(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "N", "groups", "Cin", "C", "K", "Kp", "Tc", "Vc", "T", "V", "rep", "res_kind", "bn_t", "dir", "prev",
        "wg_aligned", "wr_aligned", "wt_aligned")]


class _GenBlockForm(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("geometry", "mfma0", "mfma1", "mv0", "mv1", "lds_bytes", "grid_x")]


MMD_MAX_BW = 16


class _MmdArgs(C.Structure):
    _fields_ = [("x", c_f32p), ("x_sp", C.c_int64), ("x_sd", C.c_int64), ("x_sg", C.c_int64), ("x_sc", C.c_int64),
                ("y", c_f32p), ("y_sp", C.c_int64), ("y_sd", C.c_int64), ("y_sg", C.c_int64), ("y_sc", C.c_int64),
                ("m", C.c_int32), ("n", C.c_int32), ("dim", C.c_int32),
                ("groups", C.c_int32), ("classes", C.c_int32), ("nbw", C.c_int32),
                ("bw", C.c_double * MMD_MAX_BW),
                ("mmd2", c_f32p), ("mmd", c_f32p), ("result", c_f32p), ("mean", c_f32p),
                ("ws", C.c_void_p), ("ws_bytes", C.c_int64)]

PRDC_MAX_K = 32
PRDC_MAX_POINTS = 32768


class _PrdcArgs(C.Structure):
    _fields_ = [("real", c_f32p), ("r_sc", C.c_int64), ("r_sp", C.c_int64), ("r_so", C.c_int64),
                ("fake", c_f32p), ("f_sc", C.c_int64), ("f_sp", C.c_int64), ("f_so", C.c_int64),
                ("n", C.c_int32), ("m", C.c_int32), ("d_outer", C.c_int32), ("d_inner", C.c_int32),
                ("classes", C.c_int32), ("k", C.c_int32),
                ("radii_real", c_f32p), ("radii_fake", c_f32p), ("fake_hits", C.c_void_p), ("real_flags", C.c_void_p),
                ("counts", C.c_void_p), ("values", c_f32p), ("mean", c_f32p),
                ("ws", C.c_void_p), ("ws_bytes", C.c_int64)]

PRDC_MAX_SETS = 4


class _PrdcRadiiArgs(C.Structure):
    _fields_ = [("x", c_f32p), ("sc", C.c_int64), ("sp", C.c_int64), ("so", C.c_int64),
                ("n", C.c_int32), ("d_outer", C.c_int32), ("d_inner", C.c_int32), ("classes", C.c_int32), ("k", C.c_int32),
                ("radii", c_f32p)]


class _PrdcSetsArgs(C.Structure):
    _fields_ = [("real", c_f32p), ("r_sc", C.c_int64), ("r_sp", C.c_int64), ("r_so", C.c_int64),
                ("fake", c_f32p * PRDC_MAX_SETS), ("f_sc", C.c_int64), ("f_sp", C.c_int64), ("f_so", C.c_int64),
                ("nsets", C.c_int32), ("n", C.c_int32), ("m", C.c_int32), ("d_outer", C.c_int32), ("d_inner", C.c_int32),
                ("classes", C.c_int32), ("k", C.c_int32),
                ("radii_real", c_f32p), ("radii_fake", c_f32p), ("fake_hits", C.c_void_p), ("real_flags", C.c_void_p),
                ("counts", C.c_void_p), ("values", c_f32p), ("mean", c_f32p),
                ("ws", C.c_void_p), ("ws_bytes", C.c_int64)]

NN_MAX_K = 32
NN_MAX_POINTS = 1 << 24
NN_MAX_SPLIT = 32


class _NnArgs(C.Structure):
    _fields_ = [("query", c_f32p), ("q_sc", C.c_int64), ("q_sp", C.c_int64), ("q_so", C.c_int64),
                ("base", c_f32p), ("b_sc", C.c_int64), ("b_sp", C.c_int64), ("b_so", C.c_int64),
                ("Q", C.c_int32), ("N", C.c_int32), ("d_outer", C.c_int32), ("d_inner", C.c_int32),
                ("classes", C.c_int32), ("k", C.c_int32), ("exclude_self", C.c_int32),
                ("q_affine", C.c_int32), ("b_affine", C.c_int32),
                ("q_scale", C.c_float), ("q_shift", C.c_float), ("b_scale", C.c_float), ("b_shift", C.c_float),
                ("tile", C.c_int32), ("split", C.c_int32),
                ("idx", C.c_void_p), ("d2", c_f32p),
                ("ws", C.c_void_p), ("ws_bytes", C.c_int64)]

NN_MAX_SETS = 4
NN_SCORES_MAX_CLASSES = 1024


class _NnSetsArgs(C.Structure):
    _fields_ = [("query", c_f32p * NN_MAX_SETS), ("q_sc", C.c_int64), ("q_sp", C.c_int64), ("q_so", C.c_int64),
                ("nsets", C.c_int32),
                ("base", c_f32p), ("b_sc", C.c_int64), ("b_sp", C.c_int64), ("b_so", C.c_int64),
                ("Q", C.c_int32), ("N", C.c_int32), ("d_outer", C.c_int32), ("d_inner", C.c_int32),
                ("classes", C.c_int32), ("k", C.c_int32),
                ("q_affine", C.c_int32), ("b_affine", C.c_int32),
                ("q_scale", C.c_float), ("q_shift", C.c_float), ("b_scale", C.c_float), ("b_shift", C.c_float),
                ("tile", C.c_int32), ("split", C.c_int32),
                ("idx", C.c_void_p), ("d2", c_f32p),
                ("ws", C.c_void_p), ("ws_bytes", C.c_int64)]


NN_NORM_PARTS = 64


class _NnGramArgs(C.Structure):
    _fields_ = [("query", c_f32p * NN_MAX_SETS), ("q_sc", C.c_int64), ("q_sp", C.c_int64), ("q_so", C.c_int64),
                ("nsets", C.c_int32),
                ("base", c_f32p), ("b_sc", C.c_int64), ("b_sp", C.c_int64), ("b_so", C.c_int64),
                ("Q", C.c_int32), ("N", C.c_int32), ("d_outer", C.c_int32), ("d_inner", C.c_int32),
                ("classes", C.c_int32), ("k", C.c_int32), ("exclude_self", C.c_int32),
                ("q_affine", C.c_int32), ("b_affine", C.c_int32),
                ("q_scale", C.c_float), ("q_shift", C.c_float), ("b_scale", C.c_float), ("b_shift", C.c_float),
                ("cand", C.c_int32), ("tile", C.c_int32), ("split", C.c_int32),
                ("b_norms", c_f32p), ("b_norm_parts", c_f32p),
                ("idx", C.c_void_p), ("d2", c_f32p), ("stats", C.c_void_p),
                ("ws", C.c_void_p), ("ws_bytes", C.c_int64)]


class _NnScoresArgs(C.Structure):
    _fields_ = [("nsets", C.c_int32), ("Q", C.c_int32), ("N", C.c_int32), ("n_classes", C.c_int32),
                ("ld", C.c_int64),
                ("idx", C.c_void_p), ("d2", c_f32p),
                ("query_labels", C.c_void_p), ("base_labels", C.c_void_p), ("base_loo", c_f32p),
                ("counts", C.c_void_p), ("counts_per_class", C.c_void_p),
                ("scores64", C.c_void_p), ("scores", c_f32p)]

FRECHET_MAX_DIM = 96


class _FrechetArgs(C.Structure):
    _fields_ = [("real", c_f32p), ("r_sc", C.c_int64), ("r_ss", C.c_int64), ("r_sf", C.c_int64), ("r_so", C.c_int64),
                ("fake", c_f32p), ("f_sc", C.c_int64), ("f_ss", C.c_int64), ("f_sf", C.c_int64), ("f_so", C.c_int64),
                ("n", C.c_int32), ("m", C.c_int32), ("frames", C.c_int32), ("diff", C.c_int32),
                ("d_outer", C.c_int32), ("d_inner", C.c_int32), ("classes", C.c_int32),
                ("values", C.c_void_p), ("terms", C.c_void_p), ("mean", C.c_void_p), ("sweeps", C.c_void_p),
                ("mu_real", C.c_void_p), ("mu_fake", C.c_void_p), ("cov_real", C.c_void_p), ("cov_fake", C.c_void_p),
                ("ws", C.c_void_p), ("ws_bytes", C.c_int64)]

FRECHET_MAX_SETS = 4


class _FrechetRealArgs(C.Structure):
    _fields_ = [("real", c_f32p), ("r_sc", C.c_int64), ("r_ss", C.c_int64), ("r_sf", C.c_int64), ("r_so", C.c_int64),
                ("n", C.c_int32), ("frames", C.c_int32), ("diff", C.c_int32),
                ("d_outer", C.c_int32), ("d_inner", C.c_int32), ("classes", C.c_int32),
                ("mu_real", C.c_void_p), ("tr_real", C.c_void_p), ("G", C.c_void_p), ("sweeps_real", C.c_void_p),
                ("ws", C.c_void_p), ("ws_bytes", C.c_int64)]


class _FrechetSetsArgs(C.Structure):
    _fields_ = [("fake", c_f32p * FRECHET_MAX_SETS), ("f_sc", C.c_int64), ("f_ss", C.c_int64), ("f_sf", C.c_int64),
                ("f_so", C.c_int64),
                ("nsets", C.c_int32), ("m", C.c_int32), ("frames", C.c_int32), ("diff", C.c_int32),
                ("d_outer", C.c_int32), ("d_inner", C.c_int32), ("classes", C.c_int32),
                ("mu_real", C.c_void_p), ("tr_real", C.c_void_p), ("G", C.c_void_p),
                ("values", C.c_void_p), ("terms", C.c_void_p), ("sweeps", C.c_void_p), ("mean", C.c_void_p),
                ("mean32", c_f32p),
                ("ws", C.c_void_p), ("ws_bytes", C.c_int64)]

KIN_DESC = 6
KIN_MAX_JOINTS, KIN_MAX_BONES, KIN_MAX_MIRROR = 32, 32, 16
KIN_MIN_FRAMES = 4
KIN_MAX_ELEMS = 32768
KIN_MAX_SETS = 4
KIN_MAX_POINTS = 16384


class _KinDescArgs(C.Structure):
    _fields_ = [("x", c_f32p), ("sc", C.c_int64), ("ss", C.c_int64), ("sf", C.c_int64), ("so", C.c_int64),
                ("n", C.c_int32), ("T", C.c_int32), ("C", C.c_int32), ("V", C.c_int32), ("classes", C.c_int32),
                ("B", C.c_int32), ("M", C.c_int32),
                ("bones", C.c_void_p), ("mirror", C.c_void_p), ("still_eps", C.c_double),
                ("desc", c_f32p), ("degenerate", C.c_void_p),
                ("ws", c_f32p), ("ws_bytes", C.c_int64), ("counters", C.c_void_p), ("counters_len", C.c_int32)]


class _KinDescSetsArgs(C.Structure):
    _fields_ = [("x", c_f32p * KIN_MAX_SETS), ("sc", C.c_int64), ("ss", C.c_int64), ("sf", C.c_int64), ("so", C.c_int64),
                ("nsets", C.c_int32),
                ("n", C.c_int32), ("T", C.c_int32), ("C", C.c_int32), ("V", C.c_int32), ("classes", C.c_int32),
                ("B", C.c_int32), ("M", C.c_int32),
                ("bones", C.c_void_p), ("mirror", C.c_void_p), ("still_eps", C.c_double),
                ("desc", c_f32p * KIN_MAX_SETS), ("degenerate", C.c_void_p),
                ("ws", c_f32p), ("ws_bytes", C.c_int64), ("counters", C.c_void_p), ("counters_len", C.c_int32)]


class _KinScoresArgs(C.Structure):
    _fields_ = [("real", c_f32p), ("fake", c_f32p * KIN_MAX_SETS),
                ("nsets", C.c_int32), ("n", C.c_int32), ("m", C.c_int32), ("classes", C.c_int32),
                ("mean_real", C.c_void_p), ("mean_fake", C.c_void_p), ("w1", C.c_void_p), ("w1_mean", C.c_void_p),
                ("scores", c_f32p), ("nonfinite", C.c_void_p)]

PROJ_MAX_CHANNELS, PROJ_MAX_JOINTS, PROJ_CHUNK_FRAMES = 3, 32, 32


class _ProjLossArgs(C.Structure):
    _fields_ = [("x", c_f32p), ("x_sn", C.c_int64), ("x_sc", C.c_int64), ("x_st", C.c_int64),
                ("y", c_f32p), ("y_sn", C.c_int64), ("y_sc", C.c_int64), ("y_st", C.c_int64),
                ("scale", C.c_float), ("shift", C.c_float),
                ("m", c_f32p), ("sm", C.c_int64),
                ("n", C.c_int32), ("C", C.c_int32), ("T", C.c_int32), ("V", C.c_int32), ("B", C.c_int32),
                ("bones", C.c_void_p),
                ("lambda_pos", C.c_double), ("lambda_vel", C.c_double), ("lambda_bone", C.c_double),
                ("loss", c_f32p), ("gx", c_f32p)]


class _ProjStepArgs(C.Structure):
    _fields_ = [("w", c_f32p), ("am", c_f32p), ("av", c_f32p), ("gw", c_f32p), ("wmean", c_f32p),
                ("labels", C.c_void_p), ("loss", c_f32p), ("step", C.c_void_p),
                ("best_obj", c_f32p), ("best_loss", c_f32p), ("best_w", c_f32p), ("hist", c_f32p), ("nonfinite", C.c_void_p),
                ("n", C.c_int32), ("D", C.c_int32), ("K", C.c_int32), ("S", C.c_int32),
                ("ramp_up", C.c_int32), ("ramp_down", C.c_int32),
                ("lambda_w", C.c_double), ("lr", C.c_double), ("b1", C.c_double), ("b2", C.c_double), ("eps", C.c_double)]


STEP_MAX_PLANES = 8
STREAM_Z, STREAM_ALPHA, STREAM_NOISE_D, STREAM_NOISE_G = 0, 1, 2, 3


class _StepInputsArgs(C.Structure):
    _fields_ = [("step", C.c_void_p), ("ticket", C.c_void_p), ("seed", C.c_uint64),
                ("rank", C.c_int32), ("world", C.c_int32), ("B", C.c_int32),
                ("C", C.c_int32), ("T", C.c_int32), ("V", C.c_int32),
                ("data", c_f32p), ("d_sN", C.c_int64), ("d_sC", C.c_int64), ("d_sT", C.c_int64), ("d_sV", C.c_int64),
                ("n_rows", C.c_int64), ("label_src", C.c_void_p),
                ("perm", C.c_void_p), ("perm_stride", C.c_int64), ("batches_per_epoch", C.c_int64),
                ("scale", C.c_float), ("shift", C.c_float),
                ("real", c_f32p), ("labels", C.c_void_p),
                ("z", c_f32p), ("latent", C.c_int32), ("alpha", c_f32p),
                ("noise", c_f32p), ("n_planes", C.c_int32), ("plane_len", C.c_int64 * STEP_MAX_PLANES)]

BN_EVAL_MAX_JOBS = 8
STREAM_SAMPLE = 0x100        # word 1 of the sampler's Philox counters: STREAM_SAMPLE + (0 = z, 1 = noise, 2 = truncation draws)


class _BnEvalJob(C.Structure):
    _fields_ = [("C", C.c_int32), ("gamma", c_f32p), ("beta", c_f32p), ("running_mean", c_f32p), ("running_var", c_f32p),
                ("eps", C.c_float), ("coef", c_f32p)]


class _GenBlockInferArgs(C.Structure):
    _fields_ = [("N", C.c_int32),
                ("Cin", C.c_int32), ("C", C.c_int32), ("K", C.c_int32), ("Kp", C.c_int32),
                ("Tc", C.c_int32), ("Vc", C.c_int32), ("T", C.c_int32), ("V", C.c_int32), ("rep", C.c_int32),
                ("res_kind", C.c_int32), ("act", C.c_int32), ("slope", C.c_float),
                ("x", _Plane),
                ("wg", c_f32p), ("wr", c_f32p), ("br", c_f32p), ("wt", c_f32p), ("bt", c_f32p),
                ("b", c_f32p), ("u", c_f32p),
                ("coef_t", c_f32p), ("coef_r", c_f32p),
                ("noise", c_f32p), ("nw", c_f32p), ("out", _Plane)]


class _SampleInputsArgs(C.Structure):
    _fields_ = [("step", C.c_void_p), ("ticket", C.c_void_p), ("seed", C.c_uint64),
                ("B", C.c_int32), ("latent", C.c_int32), ("z", c_f32p),
                ("noise", c_f32p), ("noise_len", C.c_int64),
                ("t", c_f32p), ("t_rows", C.c_int32), ("t_cols", C.c_int32)]

GEN_ADJ_MAX_JOBS = 8
EVAL_MAX_SCORES = 8
COPY_IF_MAX_JOBS = 32


def _eval_record_struct(name: str, most: int, sense: bool):
    """KgEvalRecordArgs / KgEvalRecord2Args / KgEvalRecord3Args: one field list, room for ``most`` scores, ``maximise`` last"""
    fields = [("scores", c_f32p * most), ("nscores", C.c_int32), ("select", C.c_int32),
              ("iter", C.c_void_p), ("count", C.c_void_p), ("ring_val", c_f32p), ("ring_iter", C.c_void_p),
              ("ring_len", C.c_int64), ("best_val", c_f32p), ("best_iter", C.c_void_p), ("flag", C.c_void_p)]
    return type(name, (C.Structure,), {"_fields_": fields + ([("maximise", C.c_int32)] if sense else [])})


EVAL2_MAX_SCORES = 32
EVAL3_MAX_SCORES = 64
_EvalRecordArgs = _eval_record_struct("_EvalRecordArgs", EVAL_MAX_SCORES, False)
_EvalRecord2Args = _eval_record_struct("_EvalRecord2Args", EVAL2_MAX_SCORES, True)
_EvalRecord3Args = _eval_record_struct("_EvalRecord3Args", EVAL3_MAX_SCORES, True)


class _CopyJob(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("nwords", C.c_int64)]


CLS_TILE = 4
CLS_MAX_C = 1024
CLS_MAX_CLASSES = 1024


class _ClsHeadArgs(C.Structure):
    _fields_ = [("N", C.c_int32), ("C", C.c_int32), ("T", C.c_int32), ("V", C.c_int32), ("F", C.c_int32), ("L", C.c_int32),
                ("h", c_f32p), ("h_sN", C.c_int64), ("h_sC", C.c_int64),
                ("w1", c_f32p), ("b1", c_f32p), ("w2", c_f32p), ("b2", c_f32p),
                ("labels", C.c_void_p),
                ("slope", C.c_float), ("masked", C.c_int32),
                ("pooled", c_f32p), ("feat", c_f32p), ("logits", c_f32p), ("loss_per_sample", c_f32p),
                ("pred", C.c_void_p), ("loss", c_f32p), ("correct", C.c_void_p),
                ("gtop", c_f32p),
                ("g", c_f32p), ("g_sN", C.c_int64), ("g_sC", C.c_int64),
                ("dw1", c_f32p), ("db1", c_f32p), ("dw2", c_f32p), ("db2", c_f32p), ("accumulate", C.c_int32),
                ("ws", C.c_void_p), ("ws_bytes", C.c_int64)]


CLS_MAX_SETS = 4


class _ClsScoresArgs(C.Structure):
    _fields_ = [("nsets", C.c_int32), ("N", C.c_int32), ("F", C.c_int32), ("K", C.c_int32), ("Sd", C.c_int32), ("Sl", C.c_int32),
                ("feat_ld", C.c_int64),
                ("feat", c_f32p * CLS_MAX_SETS), ("pred", C.c_void_p * CLS_MAX_SETS),
                ("labels", C.c_void_p), ("div_pairs", C.c_void_p), ("mm_pairs", C.c_void_p),
                ("dist", C.c_void_p), ("scores64", C.c_void_p), ("scores", c_f32p),
                ("correct", C.c_void_p), ("correct_per_class", C.c_void_p), ("count_per_class", C.c_void_p)]


EXPORTS = {
    "kg_abi_version": (C.c_int, []),
    "kg_arch": (C.c_char_p, []),
    "kg_last_error": (C.c_char_p, []),
    "kg_reload_env": (None, []),
    "kg_peak_mfma_f32": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_double), C.c_void_p]),
    "kg_peak_copy": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "kg_conv_workspace_bytes": (C.c_int64, [C.POINTER(_ConvArgs)]),
    "kg_conv_plan_info": (C.c_int, [C.POINTER(_ConvArgs), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "kg_conv_form_info": (C.c_int, [C.POINTER(_ConvArgs), C.POINTER(_ConvFormInfo)]),
    "kg_conv_many_form": (C.c_int, [C.POINTER(_ConvArgs), C.c_int32, C.POINTER(_ConvManyForm)]),
    "kg_conv": (C.c_int, [C.POINTER(_ConvArgs), C.c_void_p]),
    "kg_conv_pack_bytes": (C.c_int64, [C.POINTER(_ConvArgs)]),
    "kg_conv_pack": (C.c_int, [C.POINTER(_ConvArgs), C.c_void_p, C.c_int64, C.c_void_p]),
    "kg_conv_many": (C.c_int, [C.POINTER(_ConvArgs), C.c_int32, C.c_void_p]),
    "kg_conv_many_plan": (C.c_int, [C.POINTER(_ConvArgs), C.c_int32, C.POINTER(C.c_int32)]),
    "kg_wgrad_workspace_bytes": (C.c_int64, [C.POINTER(_WgradArgs)]),
    "kg_wgrad": (C.c_int, [C.POINTER(_WgradArgs), C.c_void_p]),
    "kg_wgrad_plan_info": (C.c_int, [C.POINTER(_WgradArgs), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "kg_wgrad_reduce_many": (C.c_int, [C.POINTER(_WgradReduceJobs), C.c_void_p]),
    "kg_wgrad_many_workspace_bytes": (C.c_int64, [C.POINTER(_WgradArgs), C.c_int32]),
    "kg_wgrad_many": (C.c_int, [C.POINTER(_WgradArgs), C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]),
    "kg_wgrad_many_plan": (C.c_int, [C.POINTER(_WgradArgs), C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "kg_aggconv_supported": (C.c_int, [C.POINTER(_AggConvArgs)]),
    "kg_aggconv": (C.c_int, [C.POINTER(_AggConvArgs), C.c_void_p]),
    "kg_aggconv_plan_info": (C.c_int, [C.POINTER(_AggConvArgs), C.c_int32, C.POINTER(_AggConvPlanInfo)]),
    "kg_agg_plan_info": (C.c_int, [C.POINTER(_AggArgs), C.c_int32, C.POINTER(_AggPlanInfo)]),
    "kg_agg_outer_many_plan": (C.c_int, [C.POINTER(_AggArgs), C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "kg_agg_expand": (C.c_int, [C.POINTER(_AggArgs), C.c_void_p]),
    "kg_agg_reduce": (C.c_int, [C.POINTER(_AggArgs), C.c_void_p]),
    "kg_agg_outer_workspace_bytes": (C.c_int64, [C.POINTER(_AggArgs)]),
    "kg_agg_outer": (C.c_int, [C.POINTER(_AggArgs), C.c_void_p]),
    "kg_agg_outer_slabs": (C.c_int, [C.POINTER(_AggArgs)]),
    "kg_agg_outer_many": (C.c_int, [C.POINTER(_AggArgs), C.c_int32, C.c_void_p]),
    "kg_agg_outer_sum_many": (C.c_int, [C.POINTER(_OuterSumJobs), C.c_void_p]),
    "kg_gen_expand": (C.c_int, [C.POINTER(_GenArgs), C.c_void_p]),
    "kg_gen_fold": (C.c_int, [C.POINTER(_GenArgs), C.c_void_p]),
    "kg_gen_adj_finish": (C.c_int, [C.POINTER(_GenAdjJob), C.c_int32, C.c_void_p]),
    "kg_gen_tail_workspace_bytes": (C.c_int64, [C.POINTER(_GenTailArgs)]),
    "kg_gen_tail_stats": (C.c_int, [C.POINTER(_GenTailArgs), C.c_void_p]),
    "kg_gen_tail_apply": (C.c_int, [C.POINTER(_GenTailArgs), C.c_void_p]),
    "kg_gen_adj_prepare": (C.c_int, [C.POINTER(_GenPrepJob), C.c_int32, C.c_void_p]),
    "kg_genblock_lds_bytes": (C.c_int64, [C.POINTER(_GenBlockArgs)]),
    "kg_genblock_workspace_bytes": (C.c_int64, [C.POINTER(_GenBlockArgs)]),
    "kg_genblock_fwd": (C.c_int, [C.POINTER(_GenBlockArgs), C.c_void_p]),
    "kg_genblock_bwd_lds_bytes": (C.c_int64, [C.POINTER(_GenBlockBwdArgs)]),
    "kg_genblock_bwd_workspace_bytes": (C.c_int64, [C.POINTER(_GenBlockBwdArgs)]),
    "kg_genblock_bwd": (C.c_int, [C.POINTER(_GenBlockBwdArgs), C.c_void_p]),
    "kg_genblock_form": (C.c_int, [C.POINTER(_GenBlockFormQuery), C.POINTER(_GenBlockForm)]),
    "kg_head_fwd": (C.c_int, [C.POINTER(_HeadArgs), C.c_void_p]),
    "kg_head_bwd": (C.c_int, [C.POINTER(_HeadArgs), C.c_void_p]),
    "kg_head_wgrad": (C.c_int, [C.POINTER(_HeadArgs), C.c_void_p]),
    "kg_linear_fwd": (C.c_int, [C.POINTER(_LinearArgs), C.c_void_p]),
    "kg_linear_bwd": (C.c_int, [C.POINTER(_LinearArgs), C.c_void_p]),
    "kg_embed_bwd": (C.c_int, [C.POINTER(_LinearArgs), C.c_void_p]),
    "kg_label_bias_fwd": (C.c_int, [C.POINTER(_LabelBiasArgs), C.c_void_p]),
    "kg_label_bias_workspace_bytes": (C.c_int64, [C.POINTER(_LabelBiasArgs)]),
    "kg_label_bias_bwd": (C.c_int, [C.POINTER(_LabelBiasArgs), C.c_void_p]),
    "kg_aggconv_label": (C.c_int, [C.POINTER(_AggConvArgs), C.POINTER(_LabelBiasArgs), C.c_void_p]),
    "kg_mix3": (C.c_int, [C.POINTER(_MixArgs), C.c_void_p]),
    "kg_masked_adj_fwd": (C.c_int, [C.POINTER(_MaskedAdjArgs), C.c_void_p]),
    "kg_masked_adj_bwd": (C.c_int, [C.POINTER(_MaskedAdjArgs), C.c_void_p]),
    "kg_rowsum_workspace_bytes": (C.c_int64, [C.POINTER(_RowsumArgs)]),
    "kg_rowsum": (C.c_int, [C.POINTER(_RowsumArgs), C.c_void_p]),
    "kg_rowsum_many_workspace_bytes": (C.c_int64, [C.POINTER(_RowsumArgs), C.c_int32]),
    "kg_rowsum_many": (C.c_int, [C.POINTER(_RowsumArgs), C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]),
    "kg_bn_fwd": (C.c_int, [C.POINTER(_BnArgs), C.c_void_p]),
    "kg_bn_bwd_many_workspace_bytes": (C.c_int64, [C.POINTER(_BnArgs), C.c_int32]),
    "kg_bn_bwd_many": (C.c_int, [C.POINTER(_BnArgs), C.c_int32, c_f32p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p]),
    "kg_bn_fwd_many_workspace_bytes": (C.c_int64, [C.POINTER(_BnJob), C.c_int32]),
    "kg_bn_fwd_many": (C.c_int, [C.POINTER(_BnJob), C.c_int32, c_f32p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p]),
    "kg_bn_bwd": (C.c_int, [C.POINTER(_BnArgs), C.c_void_p]),
    "kg_gp_fwd": (C.c_int, [C.POINTER(_GpArgs), C.c_void_p]),
    "kg_gp_bwd": (C.c_int, [C.POINTER(_GpArgs), C.c_void_p]),
    "kg_act_bwd": (C.c_int, [C.POINTER(_EltArgs), C.c_void_p]),
    "kg_affine_act": (C.c_int, [C.POINTER(_EltArgs), C.c_void_p]),
    "kg_comm_unique_id": (C.c_int, [C.c_void_p]),
    "kg_comm_init": (C.c_int, [C.POINTER(C.c_void_p), C.c_int32, C.c_int32, C.c_void_p, C.c_int32]),
    "kg_comm_world": (C.c_int, [C.c_void_p]),
    "kg_allreduce_flat": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "kg_comm_destroy": (C.c_int, [C.c_void_p]),
    "kg_adam_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_float,
                               C.c_float, C.c_float, C.c_void_p, C.c_float, C.c_void_p]),
    "kg_mmd_workspace_bytes": (C.c_int64, [C.POINTER(_MmdArgs)]),
    "kg_mmd": (C.c_int, [C.POINTER(_MmdArgs), C.c_void_p]),
    "kg_prdc_workspace_bytes": (C.c_int64, [C.POINTER(_PrdcArgs)]),
    "kg_prdc": (C.c_int, [C.POINTER(_PrdcArgs), C.c_void_p]),
    "kg_prdc_radii": (C.c_int, [C.POINTER(_PrdcRadiiArgs), C.c_void_p]),
    "kg_prdc_sets_workspace_bytes": (C.c_int64, [C.POINTER(_PrdcSetsArgs)]),
    "kg_prdc_sets": (C.c_int, [C.POINTER(_PrdcSetsArgs), C.c_void_p]),
    "kg_nn_workspace_bytes": (C.c_int64, [C.POINTER(_NnArgs)]),
    "kg_nn": (C.c_int, [C.POINTER(_NnArgs), C.c_void_p]),
    "kg_nn_sets_workspace_bytes": (C.c_int64, [C.POINTER(_NnSetsArgs)]),
    "kg_nn_sets": (C.c_int, [C.POINTER(_NnSetsArgs), C.c_void_p]),
    "kg_nn_scores": (C.c_int, [C.POINTER(_NnScoresArgs), C.c_void_p]),
    "kg_nn_norms": (C.c_int, [C.POINTER(_NnGramArgs), C.c_void_p, C.c_void_p, C.c_void_p]),
    "kg_nn_gram_workspace_bytes": (C.c_int64, [C.POINTER(_NnGramArgs)]),
    "kg_nn_gram": (C.c_int, [C.POINTER(_NnGramArgs), C.c_void_p]),
    "kg_frechet_workspace_bytes": (C.c_int64, [C.POINTER(_FrechetArgs)]),
    "kg_frechet": (C.c_int, [C.POINTER(_FrechetArgs), C.c_void_p]),
    "kg_frechet_real_workspace_bytes": (C.c_int64, [C.POINTER(_FrechetRealArgs)]),
    "kg_frechet_real": (C.c_int, [C.POINTER(_FrechetRealArgs), C.c_void_p]),
    "kg_frechet_sets_workspace_bytes": (C.c_int64, [C.POINTER(_FrechetSetsArgs)]),
    "kg_frechet_sets": (C.c_int, [C.POINTER(_FrechetSetsArgs), C.c_void_p]),
    "kg_step_inputs": (C.c_int, [C.POINTER(_StepInputsArgs), C.c_void_p]),
    "kg_loss_append": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "kg_adam_step_fused": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_float,
                                     C.c_float, C.c_float, C.c_void_p, C.c_float, C.c_int32, C.c_void_p]),
    "kg_adam_step_ema": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_float,
                                   C.c_float, C.c_float, C.c_void_p, C.c_float, C.c_int32, C.c_float, C.c_float, C.c_void_p]),
    "kg_bn_eval_coef": (C.c_int, [C.POINTER(_BnEvalJob), C.c_int32, C.c_void_p]),
    "kg_genblock_infer_lds_bytes": (C.c_int64, [C.POINTER(_GenBlockInferArgs)]),
    "kg_genblock_infer": (C.c_int, [C.POINTER(_GenBlockInferArgs), C.c_void_p]),
    "kg_sample_inputs": (C.c_int, [C.POINTER(_SampleInputsArgs), C.c_void_p]),
    "kg_trunc_lerp": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_float,
                                C.c_void_p]),
    "kg_eval_record": (C.c_int, [C.POINTER(_EvalRecordArgs), C.c_void_p]),
    "kg_eval_record2": (C.c_int, [C.POINTER(_EvalRecord2Args), C.c_void_p]),
    "kg_eval_record3": (C.c_int, [C.POINTER(_EvalRecord3Args), C.c_void_p]),
    "kg_copy_if": (C.c_int, [C.c_void_p, C.POINTER(_CopyJob), C.c_int32, C.c_void_p]),
    "kg_cls_head_workspace_bytes": (C.c_int64, [C.POINTER(_ClsHeadArgs)]),
    "kg_cls_head_fwd": (C.c_int, [C.POINTER(_ClsHeadArgs), C.c_void_p]),
    "kg_cls_head_bwd": (C.c_int, [C.POINTER(_ClsHeadArgs), C.c_void_p]),
    "kg_cls_head_wgrad": (C.c_int, [C.POINTER(_ClsHeadArgs), C.c_void_p]),
    "kg_cls_scores": (C.c_int, [C.POINTER(_ClsScoresArgs), C.c_void_p]),
    "kg_kin_desc_workspace_bytes": (C.c_int64, [C.POINTER(_KinDescArgs)]),
    "kg_kin_desc_lds_bytes": (C.c_int64, [C.POINTER(_KinDescArgs)]),
    "kg_kin_desc": (C.c_int, [C.POINTER(_KinDescArgs), C.c_void_p]),
    "kg_kin_desc_sets_workspace_bytes": (C.c_int64, [C.POINTER(_KinDescSetsArgs)]),
    "kg_kin_desc_sets_lds_bytes": (C.c_int64, [C.POINTER(_KinDescSetsArgs)]),
    "kg_kin_desc_sets": (C.c_int, [C.POINTER(_KinDescSetsArgs), C.c_void_p]),
    "kg_kin_scores_lds_bytes": (C.c_int64, [C.POINTER(_KinScoresArgs)]),
    "kg_kin_scores": (C.c_int, [C.POINTER(_KinScoresArgs), C.c_void_p]),
    "kg_proj_loss": (C.c_int, [C.POINTER(_ProjLossArgs), C.c_void_p]),
    "kg_proj_step": (C.c_int, [C.POINTER(_ProjStepArgs), C.c_void_p]),
}

_lib = None


def load_library():
    """dlopen libkgan_hip.so (built in-tree by build.py) and declare every exported symbol."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback for the st_gcn path.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in EXPORTS.items():
        fn = getattr(lib, name)          # AttributeError if a declared symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if lib.kg_abi_version() != ABI_VERSION:
        raise RuntimeError("libkgan_hip.so ABI version mismatch")
    _lib = lib
    return lib


def _check(rc: int, what: str):
    if rc != 0:
        msg = load_library().kg_last_error().decode()
        raise RuntimeError(f"{what} failed (rc={rc}): {msg}")


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def peak_mfma_f32(sink: torch.Tensor, iters: int) -> float:
    """Enqueue the fp32-MFMA peak probe (kg_peak_mfma_f32); returns the flops of the launch."""
    fl = C.c_double(0.0)
    _check(load_library().kg_peak_mfma_f32(sink.data_ptr(), int(iters), C.byref(fl), _stream()), "kg_peak_mfma_f32")
    return fl.value


def peak_copy(src: torch.Tensor, dst: torch.Tensor) -> int:
    """Enqueue the float4 copy probe (kg_peak_copy); returns the bytes it moves (read + write)."""
    n = src.numel()
    _check(load_library().kg_peak_copy(src.data_ptr(), dst.data_ptr(), n, _stream()), "kg_peak_copy")
    return 8 * n


def reload_env():
    """Tests / tuning: make the library read its KG_* environment switches again (it reads them once at load)."""
    load_library().kg_reload_env()


SYNC_LEN = 8192
_sync_bufs = {}


def _sync_buffer(device) -> torch.Tensor:
    """Zeroed ticket counters of the last-arriver kernels (kg_bn_fwd_many, kg_bn_bwd_many, kg_gen_tail_stats, kg_genblock_fwd,
    kg_genblock_bwd, in-kernel K-split completion of kg_conv / kg_conv_many; csrc/kg_handoff.h): one buffer per (device, stream) -
    launches of one stream run one after the other, and every launch leaves its counters at zero again."""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    buf = _sync_bufs.get(key)
    if buf is None:
        buf = _sync_bufs[key] = torch.zeros(SYNC_LEN, dtype=torch.int32, device=device)
    return buf


# ---- plane tensor helpers -------------------------------------------------------------------------

def is_plane(x: torch.Tensor) -> bool:
    if x.dim() != 4:
        return False
    n, c, t, v = x.shape
    return (v == 1 or x.stride(3) == 1) and (t == 1 or x.stride(2) == v)


def as_plane(x: torch.Tensor) -> torch.Tensor:
    """Return x itself if its (t,v) plane is contiguous, else a channel-major copy."""
    if x.dtype != torch.float32:
        raise TypeError(f"st_gcn path is fp32 only, got {x.dtype}")
    if is_plane(x):
        return x
    out = new_plane(x.shape[0], x.shape[1], x.shape[2], x.shape[3], x.device)
    out.copy_(x)
    return out


# floats of slack in front of every plane tensor we allocate.  No kernel needs it any more: the 128-bit-load forms of kg_conv
# that read up to one frame in front of a row are retired (kg_conv.hip, "plan tile codes"), every remaining load path is
# bounds-selected per tap and tests/test_guarded_gpu.py runs kg_conv / kg_aggconv / kg_wgrad on operands with lead 0 between
# poisoned red zones.  Kept (128 bytes per tensor) so that KgConvGroup.x_lead reports what it always did; DESIGN.md 14.
PLANE_LEAD = 32


def new_plane(n, c, t, v, device, zero=False) -> torch.Tensor:
    """(N,C,T,V) tensor stored channel-major (C,N,T,V): every channel row is one contiguous run.  The
    storage starts PLANE_LEAD floats early (historical slack: see PLANE_LEAD, no kernel reads it)."""
    numel = c * n * t * v
    buf = (torch.zeros if zero else torch.empty)(numel + PLANE_LEAD, dtype=torch.float32, device=device)
    return buf[PLANE_LEAD:].view(c, n, t, v).permute(1, 0, 2, 3)


def _sn_sc(x: torch.Tensor):
    n, c, t, v = x.shape
    sn = x.stride(0) if n > 1 else t * v
    sc = x.stride(1) if c > 1 else t * v
    return sn, sc


def _need_cuda(*ts):
    """Every operand on the GPU, and on the CURRENT device: the launches go to the current device's current stream
    (`_stream`), so a tensor of another device would be touched by wrong-device, unordered work (round-1 ADVICE)."""
    cur = None
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("kinetic_gan_amd: the st_gcn hot path runs on the GPU only "
                               "(tensor on %s); there is no CPU fallback" % t.device)
        if cur is None:
            cur = torch.cuda.current_device()
        if t.device.index != cur:
            raise RuntimeError("kinetic_gan_amd: tensor on %s but the current device is cuda:%d - select the device "
                               "first (torch.cuda.set_device / `with torch.cuda.device(...)`)" % (t.device, cur))


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _bind(a, field: str, pre: str, t: torch.Tensor, convert: bool = False) -> torch.Tensor:
    """Bind a plane tensor to a struct: a.<field> = its pointer, a.<pre>_sN / a.<pre>_sC = its strides.  ``convert``: through
    as_plane first.  Returns the tensor that was bound - the caller holds it until the launch is enqueued."""
    if convert:
        t = as_plane(t)
    setattr(a, field, t.data_ptr())
    sn, sc = _sn_sc(t)
    setattr(a, pre + "_sN", sn)
    setattr(a, pre + "_sC", sc)
    return t


def _query(query: str, a, count: Optional[int] = None) -> int:
    """The bytes the library's size query ``query`` answers for the filled struct ``a`` (for the ``count`` structs of the array
    ``a``: the *_many launchers); an answer < 0 raises the library's message through _check."""
    fn = getattr(load_library(), query)
    nbytes = fn(C.byref(a)) if count is None else fn(a, count)
    if nbytes < 0:
        _check(-1, query)
    return nbytes


def _workspace(query: str, a, device, count: Optional[int] = None, tickets: Optional[str] = None, lazy: bool = False):
    """_query, then allocate that much fp32 scratch.  One struct: a.ws / a.ws_bytes are set, and with ``tickets`` ("counters" /
    "sync") a.<tickets> / a.<tickets>_len name the stream's ticket counters.  An array of ``count`` structs: the caller passes
    ws.data_ptr(), ws.numel() * 4 to its launcher.  ``lazy``: a launch that needs no scratch gets none - nothing is allocated
    or set (the library's plan reads these fields) and None is returned.  The caller holds the result until its launch."""
    nbytes = _query(query, a, count)
    if lazy and nbytes == 0:
        return None
    ws = torch.empty(nbytes // 4 if lazy else max(1, nbytes // 4), dtype=torch.float32, device=device)
    if count is None:
        a.ws, a.ws_bytes = ws.data_ptr(), nbytes if lazy else ws.numel() * 4
        if tickets is not None:
            sync = _sync_buffer(device)
            setattr(a, tickets, sync.data_ptr())
            setattr(a, tickets + "_len", sync.numel())
    return ws


def _dest(t: torch.Tensor, n: int, msg: str) -> torch.Tensor:
    """a destination the kernels write flat: contiguous fp32 of n elements, else ValueError(msg)"""
    if t.numel() != n or not t.is_contiguous() or t.dtype != torch.float32:
        raise ValueError(msg)
    return t


def _chunks(jobs: Sequence, most: int):
    """the job table in runs of at most ``most`` entries: one launch each"""
    for i in range(0, len(jobs), most):
        yield jobs[i:i + most]


# ---- weight addressing -------------------------------------------------------------------------------

class WView(NamedTuple):
    """W(d, m, c) = base + d*sT + (m // MB)*sMB + (m % MB)*sO + c*sI (elements)."""
    sT: int
    sO: int
    sI: int
    sMB: int = 0
    MB: int = 1 << 30


class Group(NamedTuple):
    x: torch.Tensor          # plane tensor (N, Cin or taps*Cin, T_in, V_in)
    w: torch.Tensor          # contiguous storage of the weights
    wv: WView
    Cin: int
    taps: int = 1
    tap_mode: int = TAP_TIME
    t_stride: int = 1
    transposed: bool = False
    vmap: Optional[torch.Tensor] = None    # int32 device tensor, V_out entries


last_conv_plan = None     # set to a list to have conv() report (tile, nsplit) of its last launch
last_conv_form = None     # set to a list: conv() / conv_many() append the form (a dict: family name, instantiation, geometry) of
                          # every launch, in call order - kg_conv_form_info / kg_conv_many_form on the arguments of the launch


def conv_form_dict(a) -> dict:
    """kg_conv_form_info of a filled KgConvArgs as a dict, `family` by name"""
    f = _ConvFormInfo()
    _check(load_library().kg_conv_form_info(C.byref(a), C.byref(f)), "kg_conv_form_info")
    d = plan_dict(f)
    d["family"] = CONV_FAMILY_NAMES[f.family]
    return d


def conv_many_form_dict(arr, n: int) -> dict:
    """kg_conv_many_form of n KgConvArgs as a dict (family "many"; tile -1: one kg_conv launch per job)"""
    f = _ConvManyForm()
    _check(load_library().kg_conv_many_form(arr, n, C.byref(f)), "kg_conv_many_form")
    d = plan_dict(f)
    for k in ("xcd", "wg_begin", "nwg"):
        d[k] = d[k][:n]
    d["family"] = "many"
    return d

# Executed-work accounting (bench.py: SURVEY 8d "if the build prunes ... it must also report executed FLOPs"): set
# to a dict and every launch adds the flops it really performs (2 per multiply-add, per kernel family).
flop_count = None


def _count(kind: str, flops: float):
    if flop_count is not None:
        flop_count[kind] = flop_count.get(kind, 0.0) + float(flops)


def _conv_args(groups: Sequence[Group], N: int, M: int, T_out: int, V_out: int,
               bias0=None, bias1=None, add=None, add_tstride: int = 1,
               act: int = ACT_NONE, slope: float = 0.2, mask=None, out: Optional[torch.Tensor] = None, out_t0: int = 0,
               out_tstride: int = 1, wpack: Optional[torch.Tensor] = None, alloc_out: bool = True):
    """Fill a KgConvArgs (without workspace); returns (args, out, tensors that must outlive the launch)."""
    a = _ConvArgs()
    if wpack is not None:
        _need_cuda(wpack)
        a.wpack, a.wpack_bytes = wpack.data_ptr(), wpack.numel() * wpack.element_size()
    a.N, a.M, a.T_out, a.V_out = N, M, T_out, V_out
    keep = []
    dev = groups[0].x.device
    a.ngroups = len(groups)
    for i, g in enumerate(groups):
        x = as_plane(g.x)
        w = g.w if g.w.is_contiguous() else g.w.contiguous()
        _need_cuda(x, w, g.vmap)
        keep += [x, w]
        cg = a.g[i]
        _bind(cg, "x", "x", x)
        cg.Cin, cg.T_in, cg.V_in = g.Cin, x.shape[2], x.shape[3]
        cg.x_lead = min(int(x.storage_offset()), 1 << 20)
        cg.vmap = _ptr(g.vmap)
        cg.w = w.data_ptr()
        cg.w_sT, cg.w_sO, cg.w_sI, cg.w_sMB = g.wv.sT, g.wv.sO, g.wv.sI, g.wv.sMB
        cg.w_MB = min(g.wv.MB, 1 << 30)
        cg.taps, cg.tap_mode, cg.t_stride, cg.transposed = g.taps, g.tap_mode, g.t_stride, int(g.transposed)
    if out is None and not alloc_out:
        pass                        # (kg_conv_pack / kg_conv_pack_bytes never touch the output)
    elif out is None:
        out = new_plane(N, M, T_out, V_out, dev)
        a.out = out.data_ptr()
    else:
        if (not is_plane(out) or out.shape[0] != N or out.shape[1] != M or out.shape[3] != V_out
                or out_t0 + (T_out - 1) * out_tstride >= out.shape[2] or out_tstride < 1 or out_t0 < 0):
            raise ValueError("conv: out must be a plane tensor (N, M, T, V_out) that holds frames out_t0 + to * out_tstride")
        _need_cuda(out)
        a.out = out.data_ptr() + 4 * out_t0 * V_out
        a.o_tstride = out_tstride
    if out is not None:
        a.o_sN, a.o_sC = _sn_sc(out)
    _need_cuda(bias0, bias1, add)
    a.bias0, a.bias1 = _ptr(bias0), _ptr(bias1)
    if add is not None:
        keep.append(_bind(a, "add", "a", add, True))
    a.a_tstride = add_tstride
    a.act, a.slope = act, slope
    if mask is not None:
        mask = as_plane(mask)
        _need_cuda(mask)
        if tuple(mask.shape) != (N, M, T_out, V_out):
            raise ValueError(f"conv: mask shape {tuple(mask.shape)} != output shape {(N, M, T_out, V_out)}")
        keep.append(_bind(a, "mask", "m", mask))
    _count("kg_conv", 2.0 * M * sum(g.taps * g.Cin for g in groups) * N * T_out * V_out)
    return a, out, keep


def conv_pack(groups: Sequence[Group], N: int, M: int, T_out: int, V_out: int, out: Optional[torch.Tensor] = None):
    """The groups' weights in the packed layout of kg_conv's bf16-split form (kg_conv_pack), or None when
    that form cannot run the launch.  Pass the result as ``wpack`` to conv() calls with the same groups / M (any batch
    size) until the weights change; ``out``: a buffer of an earlier call to refill in place."""
    lib = load_library()
    a, _, keep = _conv_args(groups, N, M, T_out, V_out, alloc_out=False)
    nbytes = _query("kg_conv_pack_bytes", a)
    if nbytes == 0:
        return None
    if out is None:
        out = torch.empty(nbytes // 4, dtype=torch.int32, device=groups[0].x.device)
    _check(lib.kg_conv_pack(C.byref(a), out.data_ptr(), out.numel() * 4, _stream()), "kg_conv_pack")
    return out


def conv(groups: Sequence[Group], N: int, M: int, T_out: int, V_out: int,
         bias0=None, bias1=None, add=None, add_tstride: int = 1,
         act: int = ACT_NONE, slope: float = 0.2, mask=None, out: Optional[torch.Tensor] = None, out_t0: int = 0,
         out_tstride: int = 1, wpack: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``mask``: optional (N, M, T_out, V_out) activation output; the result is multiplied by its LeakyReLU
    derivative (slope where mask <= 0) - "g * act'(out)" of the consumer folded into this launch.
    ``out`` (a plane tensor (N, M, T, V_out)), ``out_t0``, ``out_tstride``: write output frame `to` to frame
    out_t0 + to * out_tstride of `out` instead of allocating the result (returns `out`)."""
    lib = load_library()
    a, out, keep = _conv_args(groups, N, M, T_out, V_out, bias0, bias1, add, add_tstride, act, slope, mask, out, out_t0, out_tstride,
                              wpack)
    if last_conv_plan is not None:       # tests / tuning: record which kernel configuration ran
        t, ns = C.c_int32(), C.c_int32()
        lib.kg_conv_plan_info(C.byref(a), C.byref(t), C.byref(ns))
        last_conv_plan[:] = [t.value, ns.value]
    # (scratch only for a K-split launch, which completes its tiles itself through the ticket counters: no epilogue launch;
    #  ws and keep are held until the launch below is enqueued)
    ws = _workspace("kg_conv_workspace_bytes", a, groups[0].x.device, tickets="sync", lazy=True)
    if last_conv_form is not None:       # (after the workspace: the ticket counters decide the completion form)
        last_conv_form.append(conv_form_dict(a))
    _check(lib.kg_conv(C.byref(a), _stream()), "kg_conv")
    return out


CONV_MANY_MAX = 4


def conv_many(jobs: Sequence[dict]) -> list:
    """Several independent kg_conv problems (each a dict of conv()'s arguments) in one launch where the launcher's plans
    allow it (kg_conv_many), one launch each otherwise; returns the outputs in order.  No job may write what another
    job of the call reads."""
    lib = load_library()
    if len(jobs) == 1:
        return [conv(**jobs[0])]
    outs, keep = [], []          # keep: converted operands and scratch of every job, held until its launch is enqueued
    for chunk in _chunks(jobs, CONV_MANY_MAX):
        arr = (_ConvArgs * len(chunk))()
        for i, j in enumerate(chunk):
            a, out, kp = _conv_args(**j)
            # (the scratch is only used when the call falls back to one launch per job)
            keep += kp + [_workspace("kg_conv_workspace_bytes", a, out.device, tickets="sync", lazy=True)]
            arr[i] = a
            outs.append(out)
        if last_conv_plan is not None:       # tests: the shared launch's tile, or -1 (one launch per job)
            t = C.c_int32()
            lib.kg_conv_many_plan(arr, len(chunk), C.byref(t))
            last_conv_plan[:] = [t.value, 1]
        if last_conv_form is not None:       # the shared launch, or (tile -1) the single launches that replace it
            mf = conv_many_form_dict(arr, len(chunk))
            last_conv_form.append(mf)
            if mf["tile"] < 0:
                last_conv_form.extend(conv_form_dict(arr[i]) for i in range(len(chunk)))
        _check(lib.kg_conv_many(arr, len(chunk), _stream()), "kg_conv_many")
    return outs


last_wgrad_plan = None    # set to a list to have wgrad() / wgrad_many() report (tile variant, splits) of every job, in call order


def _wgrad_args(g, x, Cin, taps, tap_mode, t_stride, vmap, wv, dw, accumulate, extra, keep):
    """Fill a KgWgradArgs (without workspace) for one layer; tensors that must outlive the launch go to `keep`."""
    g = as_plane(g)
    x = as_plane(x)
    _need_cuda(g, x, vmap, dw)
    a = _WgradArgs()
    a.N, a.M, a.T_out, a.V_out = g.shape
    _bind(a, "g", "g", g)
    _bind(a, "x", "x", x)
    a.Cin, a.T_in, a.V_in = Cin, x.shape[2], x.shape[3]
    a.vmap = _ptr(vmap)
    a.taps, a.tap_mode, a.t_stride = taps, tap_mode, t_stride
    if len(extra) > 2:
        raise ValueError("wgrad: at most two extra operand pairs")
    keep += [g, x]
    for i, (ge, xe) in enumerate(extra):
        ge, xe = as_plane(ge), as_plane(xe)
        _need_cuda(ge, xe)
        if tuple(ge.shape[1:]) != tuple(g.shape[1:]) or tuple(xe.shape[1:]) != tuple(x.shape[1:]) or ge.shape[0] != xe.shape[0]:
            raise ValueError(f"wgrad: extra pair {i} has another geometry: {tuple(ge.shape)} / {tuple(xe.shape)}")
        keep += [ge, xe]
        e = a.extra[i]
        e.N = ge.shape[0]
        _bind(e, "g", "g", ge)
        _bind(e, "x", "x", xe)
    a.nextra = len(extra)
    a.dw = dw.data_ptr()
    a.accumulate = int(accumulate)
    a.w_sT, a.w_sO, a.w_sI = wv.sT, wv.sO, wv.sI
    _count("kg_wgrad", 2.0 * taps * a.M * Cin * a.T_out * a.V_out * (a.N + sum(ge.shape[0] for ge, _ in extra)))
    return a


def wgrad(g: torch.Tensor, x: torch.Tensor, Cin: int, taps: int, tap_mode: int, t_stride: int,
          vmap: Optional[torch.Tensor], w_numel: int, wv: WView, out: Optional[torch.Tensor] = None,
          accumulate: bool = False, extra=(), defer: Optional[list] = None) -> torch.Tensor:
    """Returns the flat (w_numel,) gradient buffer written with the weight's own addressing.  out: write (or, with
    accumulate, add) into this contiguous (w_numel,) fp32 tensor instead of a new one.  extra: up to two more
    (g, x) pairs of the same layer geometry (batch size may differ) whose products are summed into the same result.
    defer: a list - only the partial slabs are computed now and a job record (which keeps the workspace alive) is
    appended; wgrad_reduce_many(defer) later finishes all of them in one launch."""
    lib = load_library()
    if out is None:
        if accumulate:
            raise ValueError("wgrad: accumulate needs out")
        dw = torch.empty(w_numel, dtype=torch.float32, device=g.device)
    else:
        dw = _dest(out, w_numel, "wgrad: out must be a contiguous fp32 tensor of the weight's size")
    keep = []                # the converted operands, held until the launch is enqueued
    a = _wgrad_args(g, x, Cin, taps, tap_mode, t_stride, vmap, wv, dw, accumulate, extra, keep)
    ws = _workspace("kg_wgrad_workspace_bytes", a, g.device)
    if last_wgrad_plan is not None:      # tests / tuning: record the tile variant and the number of partial slabs
        v, ns = C.c_int32(), C.c_int32()
        _check(lib.kg_wgrad_plan_info(C.byref(a), C.byref(v), C.byref(ns)), "kg_wgrad_plan_info")
        last_wgrad_plan[:] = [(v.value, ns.value)]
    if defer is not None:
        a.defer_reduce = 1
        per = taps * a.M * Cin
        defer.append(dict(ws=ws, dw=dw, w_sT=wv.sT, w_sO=wv.sO, w_sI=wv.sI, taps=taps, M=a.M, Cin=Cin,
                          splits=max(1, ws.numel() // per), accumulate=int(accumulate)))
    _check(lib.kg_wgrad(C.byref(a), _stream()), "kg_wgrad")
    return dw


def wgrad_many(jobs: Sequence[dict]):
    """The weight gradients of several layers in shared launches (kg_wgrad_many).  Each job: dict(g, x, Cin, taps,
    tap_mode, t_stride, vmap, wv, out (contiguous fp32 destination), accumulate, extra=[(g, x), ...])."""
    lib = load_library()
    if not jobs:
        return
    arr = (_WgradArgs * len(jobs))()
    keep = []                # the converted operands of every job, held until the launch is enqueued
    for i, j in enumerate(jobs):
        dw = j["out"]
        if not dw.is_contiguous() or dw.dtype != torch.float32:
            raise ValueError("wgrad_many: out must be a contiguous fp32 tensor")
        arr[i] = _wgrad_args(j["g"], j["x"], j["Cin"], j["taps"], j["tap_mode"], j["t_stride"], j.get("vmap"),
                             j["wv"], dw, j.get("accumulate", False), j.get("extra", ()), keep)
    ws = _workspace("kg_wgrad_many_workspace_bytes", arr, jobs[0]["g"].device, len(jobs))
    if last_wgrad_plan is not None:      # tests / tuning: (tile variant, splits) of every job
        v, ns = (C.c_int32 * len(jobs))(), (C.c_int32 * len(jobs))()
        _check(lib.kg_wgrad_many_plan(arr, len(jobs), v, ns), "kg_wgrad_many_plan")
        last_wgrad_plan[:] = list(zip(v, ns))
    _check(lib.kg_wgrad_many(arr, len(jobs), ws.data_ptr(), ws.numel() * 4, _stream()), "kg_wgrad_many")


def wgrad_reduce_many(jobs: list):
    """Finish the deferred kg_wgrad calls recorded in `jobs` (see wgrad(defer=...)): one launch per 24 jobs."""
    lib = load_library()
    for chunk in _chunks(jobs, WGRAD_REDUCE_MAX_JOBS):
        js = _WgradReduceJobs()
        js.njobs = len(chunk)
        for k, j in enumerate(chunk):
            r = js.job[k]
            r.ws, r.dw = j["ws"].data_ptr(), j["dw"].data_ptr()
            r.w_sT, r.w_sO, r.w_sI = j["w_sT"], j["w_sO"], j["w_sI"]
            r.taps, r.M, r.Cin, r.splits, r.accumulate = j["taps"], j["M"], j["Cin"], j["splits"], j["accumulate"]
        _check(lib.kg_wgrad_reduce_many(C.byref(js), _stream()), "kg_wgrad_reduce_many")
    jobs.clear()


last_agg_plan = None      # set to a list: agg_expand() / agg_reduce() / agg_outer() append the plan (a dict, "op" added) of every
#                           launch, agg_outer_finish() one dict(op="outer_many", launch=[..], slabs=[..]) per call
last_aggconv_plan = None  # set to a list: aggconv() / aggconv_label() append the plan (a dict) of every launch


def _record_agg_plan(lib, a, op):
    p = _AggPlanInfo()
    _check(lib.kg_agg_plan_info(C.byref(a), op, C.byref(p)), "kg_agg_plan_info")
    last_agg_plan.append(dict(plan_dict(p), op=("expand", "reduce", "outer")[op]))


def _record_aggconv_plan(lib, a, label_J):
    p = _AggConvPlanInfo()
    _check(lib.kg_aggconv_plan_info(C.byref(a), label_J, C.byref(p)), "kg_aggconv_plan_info")
    last_aggconv_plan.append(plan_dict(p))


def _agg_args(N, Cc, K, V, W, T, rep, A):
    a = _AggArgs()
    a.N, a.C, a.K, a.V, a.W, a.T, a.rep = N, Cc, K, V, W, T, rep
    a.a = A.data_ptr()
    return a


def _adjacency(A: torch.Tensor):
    """(storage tensor, transposed flag): a (K,V,W) view of a contiguous (K,W,V) tensor is passed as it is stored"""
    if A.is_contiguous():
        return A, 0
    if A.dim() == 3 and A.transpose(1, 2).is_contiguous():
        return A.transpose(1, 2), 1
    return A.contiguous(), 0


def agg_expand(x: torch.Tensor, A: torch.Tensor, rep: int = 1) -> torch.Tensor:
    lib = load_library()
    x = as_plane(x)
    k, va, w = A.shape
    A, tr = _adjacency(A)
    _need_cuda(x, A)
    n, c, t, v = x.shape
    assert va == v, (A.shape, x.shape)
    a = _agg_args(n, c, k, v, w, t, rep, A)
    a.a_transposed = tr
    _bind(a, "x", "x", x)
    out = _bind(a, "out", "o", new_plane(n, k * c, t * rep, w, x.device))
    _count("kg_agg", 2.0 * k * v * w * c * n * t * rep)
    if last_agg_plan is not None:        # tests / tuning: record which kernel form and instantiation runs
        _record_agg_plan(lib, a, AGG_OP_EXPAND)
    _check(lib.kg_agg_expand(C.byref(a), _stream()), "kg_agg_expand")
    return out


AGGCONV_P = 4          # width of the neighbour table (kgan_hip.h)


def aggconv_supported(V: int, W: int, pcount, ncols: int) -> bool:
    """Launch geometries the fused aggregation + gcn kernel takes (mirrors kg_aggconv_supported); below ~8k columns
    the unfused pair wins (kg_conv can split K across workgroups there)."""
    span = (127 // W + 2) * V
    return span <= 384 and pcount[0] <= 1 and pcount[1] <= AGGCONV_P and pcount[2] <= 1 and ncols >= 8192


def aggconv(x: torch.Tensor, A: torch.Tensor, nbr: torch.Tensor, pcount, w: torch.Tensor, wv: WView, M: int,
            add: Optional[torch.Tensor] = None, add_tstride: int = 1, want_xa: bool = False):
    """out = sum_k W_k (x A_k) (+ add) in one launch (kg_aggconv); returns (out, xa | None), xa = the aggregated
    planes (N, K*Cin, T, W) when want_xa.  nbr: (K, W, 4) int32 neighbour table of A's fixed sparsity pattern."""
    lib = load_library()
    a, out, xa, flops, _keep = _aggconv_args(x, A, nbr, pcount, w, wv, M, add, add_tstride, want_xa)
    _count("kg_aggconv", flops)
    if last_aggconv_plan is not None:    # tests / tuning: record which kernel form and instantiation runs
        _record_aggconv_plan(lib, a, 0)
    _check(lib.kg_aggconv(C.byref(a), _stream()), "kg_aggconv")
    return out, xa


def _aggconv_args(x, A, nbr, pcount, w, wv, M, add, add_tstride, want_xa):
    x = as_plane(x)
    k, va, wd = A.shape
    A, tr = _adjacency(A)
    w = w if w.is_contiguous() else w.contiguous()
    _need_cuda(x, A, nbr, w, add)
    n, c, t, v = x.shape
    assert va == v and nbr.dtype == torch.int32 and tuple(nbr.shape) == (k, wd, AGGCONV_P), (A.shape, x.shape, nbr.shape)
    a = _AggConvArgs()
    a.N, a.Cin, a.M, a.T, a.V, a.W, a.K = n, c, M, t, v, wd, k
    _bind(a, "x", "x", x)
    a.a, a.a_transposed = A.data_ptr(), tr
    a.nbr = nbr.data_ptr()
    for i in range(3):
        a.pcount[i] = int(pcount[i]) if i < k else 0
    a.w = w.data_ptr()
    a.w_sT, a.w_sO, a.w_sI = wv.sT, wv.sO, wv.sI
    out = _bind(a, "out", "o", new_plane(n, M, t, wd, x.device))
    if add is not None:
        add = _bind(a, "add", "a", add, True)
    a.a_tstride = add_tstride
    xa = None
    if want_xa:
        xa = _bind(a, "xa", "xa", new_plane(n, k * c, t, wd, x.device))
    # (the operands are returned with the args: x / A / w / add may be converted copies that must outlive the launch)
    return a, out, xa, 2.0 * M * k * c * n * t * wd, (x, A, w, add)


def aggconv_label_supported(K: int, Cin: int, M: int, V: int, W: int, J: int) -> bool:
    """Geometries kg_aggconv_label takes (the tiny-channel form of kg_aggconv; mirrors its checks)."""
    return K <= 3 and Cin <= 4 and M <= 64 and W <= 32 and K * V * W <= 4096 and 0 < J <= 512 and K * M * J <= 12288


def aggconv_label(x: torch.Tensor, A: torch.Tensor, nbr: torch.Tensor, pcount, w: torch.Tensor, wv: WView, M: int,
                  labels: torch.Tensor, emb: torch.Tensor, wg: torch.Tensor, cin: int, J: int, want_xa: bool = False):
    """Block 0's gcn with its label bias in ONE launch (kg_aggconv_label): the result of
    aggconv(x, A, nbr, pcount, w, wv, M, add=label_bias_fwd(labels, emb, wg, K, M, cin, J, A), add_tstride=0, want_xa)
    without the bias tensor or the class-table launch.  wg: the whole gcn weight (K*M, cin, 1, 1) - its first J input
    columns multiply the label channels; w / wv address its data columns.  Returns (out, xa | None)."""
    lib = load_library()
    _need_cuda(labels, emb, wg)
    a, out, xa, flops, _keep = _aggconv_args(x, A, nbr, pcount, w, wv, M, None, 0, want_xa)
    lb = _LabelBiasArgs()
    lb.N, lb.L, lb.J, lb.K, lb.C, lb.V, lb.W = a.N, emb.shape[0], J, a.K, M, a.V, a.W
    assert emb.is_contiguous() and emb.shape[1] == J and labels.dtype == torch.int64 and labels.is_contiguous()
    assert labels.numel() == a.N and wg.is_contiguous() and wg.numel() == a.K * M * cin
    lb.labels, lb.emb = labels.data_ptr(), emb.data_ptr()
    lb.w, lb.w_sK, lb.w_sC = wg.data_ptr(), M * cin, cin
    _count("kg_aggconv", flops)
    if last_aggconv_plan is not None:
        _record_aggconv_plan(lib, a, J)
    _check(lib.kg_aggconv_label(C.byref(a), C.byref(lb), _stream()), "kg_aggconv_label")
    return out, xa


def agg_reduce(y: torch.Tensor, A: torch.Tensor, fold: int = 1, res: Optional[torch.Tensor] = None, res_tstride: int = 1,
               res_inv: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None, slope: float = 0.2) -> torch.Tensor:
    """out = sum_k y_k A_k (kg_agg_reduce).  Optional epilogue (fold = 1): ``res`` (N, C, Tr, Vr) lands on frames
    t = tr * res_tstride and on the vertices w with res_inv[w] >= 0 before the result is multiplied by the LeakyReLU
    derivative of ``mask`` (N, C, T, W): (aggregate + scatter(res)) * lrelu'(mask)."""
    lib = load_library()
    y = as_plane(y)
    k, va, w = A.shape
    A, tr = _adjacency(A)
    _need_cuda(y, A, res, res_inv, mask)
    n, kc, tin, v = y.shape
    assert va == v and kc % k == 0 and tin % fold == 0, (A.shape, y.shape, fold)
    c = kc // k
    a = _agg_args(n, c, k, v, w, tin // fold, fold, A)
    a.a_transposed = tr
    _bind(a, "x", "x", y)
    out = _bind(a, "out", "o", new_plane(n, c, tin // fold, w, y.device))
    if res is not None:
        res = as_plane(res)
        assert fold == 1 and res.shape[0] == n and res.shape[1] == c, (res.shape, out.shape)
        _bind(a, "res", "r", res)
        a.r_T, a.r_V, a.r_tstride = res.shape[2], res.shape[3], res_tstride
        a.r_inv = _ptr(res_inv)
    if mask is not None:
        mask = as_plane(mask)
        assert fold == 1 and tuple(mask.shape) == tuple(out.shape), (mask.shape, out.shape)
        _bind(a, "mask", "m", mask)
    a.slope = slope
    _count("kg_agg", 2.0 * k * v * w * c * n * tin)
    if last_agg_plan is not None:
        _record_agg_plan(lib, a, AGG_OP_REDUCE)
    _check(lib.kg_agg_reduce(C.byref(a), _stream()), "kg_agg_reduce")
    return out


def agg_outer(x: torch.Tensor, y: torch.Tensor, K: int, rep: int = 1, out: Optional[torch.Tensor] = None,
              defer: Optional[list] = None) -> torch.Tensor:
    """``out``: optional contiguous (K, V, W) fp32 destination (e.g. a slice of a packed adjacency-gradient buffer).
    ``defer``: a list - the problem is only recorded; agg_outer_finish(defer) computes all recorded problems in shared
    launches (``out`` is not valid before that)."""
    lib = load_library()
    x = as_plane(x)
    y = as_plane(y)
    _need_cuda(x, y, out)
    n, c, t, v = x.shape
    w = y.shape[3]
    assert y.shape[1] == K * c and y.shape[2] == t * rep, (x.shape, y.shape, K, rep)
    if out is None:
        out = torch.empty((K, v, w), dtype=torch.float32, device=x.device)
    elif tuple(out.shape) != (K, v, w) or not out.is_contiguous() or out.dtype != torch.float32:
        raise ValueError("agg_outer: out must be a contiguous fp32 (K, V, W) tensor")
    a = _agg_args(n, c, K, v, w, t, rep, out)
    a.a = None
    _bind(a, "x", "x", x)
    _bind(a, "y", "y", y)
    a.out = out.data_ptr()
    ws = _workspace("kg_agg_outer_workspace_bytes", a, x.device)
    _count("kg_agg", 2.0 * K * v * w * c * n * t * rep)
    if defer is not None:
        # nothing is launched now: the record keeps the operands and the scratch alive until agg_outer_finish
        defer.append(dict(args=a, keep=(x, y, ws, out)))
        return out
    if last_agg_plan is not None:
        _record_agg_plan(lib, a, AGG_OP_OUTER)
    _check(lib.kg_agg_outer(C.byref(a), _stream()), "kg_agg_outer")
    return out


def agg_outer_finish(jobs: list):
    """The deferred agg_outer problems recorded in `jobs` (the adjacency gradients of a backward pass): ONE launch
    for the matrix-core form + one for all slab sums (kg_agg_outer_many).  ``out`` of every record is valid after
    this call; x and y must not have been written since they were recorded."""
    lib = load_library()
    if jobs:
        arr = (_AggArgs * len(jobs))()
        for i, j in enumerate(jobs):
            C.memmove(C.byref(arr[i]), C.byref(j["args"]), C.sizeof(_AggArgs))
        if last_agg_plan is not None:    # tests / tuning: the shared launch and the slabs of every job
            la, ns = (C.c_int32 * len(jobs))(), (C.c_int32 * len(jobs))()
            _check(lib.kg_agg_outer_many_plan(arr, len(jobs), la, ns), "kg_agg_outer_many_plan")
            last_agg_plan.append(dict(op="outer_many", launch=list(la), slabs=list(ns)))
        _check(lib.kg_agg_outer_many(arr, len(jobs), _stream()), "kg_agg_outer_many")
    jobs.clear()


def _gen_common(a, A, U, N, Tc, Vc, V, rep, B=None):
    a.N, a.Tc, a.Vc, a.V, a.rep = N, Tc, Vc, V, rep
    if A is not None:
        a.a = A.data_ptr()
    if U is not None:
        a.u = U.data_ptr()
    if B is not None:
        if not B.is_contiguous() or B.dim() != 3 or B.shape[1] != Vc or B.shape[2] != V:
            raise ValueError("gen_expand / gen_fold: B must be a contiguous (K, Vc, V) tensor")
        a.b = B.data_ptr()


def gen_adj_prepare(jobs: Sequence[dict]):
    """A[lvl] * importance and U (A * importance) of several generator blocks in one launch (kg_gen_adj_prepare).  Each
    job: dict(a (K, V, V), imp (K, V, V) | None, u (Vc, V) | None, aeff (K, V, V) out, b (K, Vc, V) out), all
    contiguous fp32."""
    lib = load_library()
    for chunk in _chunks(jobs, GEN_ADJ_MAX_JOBS):
        arr = (_GenPrepJob * len(chunk))()
        for q, j in enumerate(chunk):
            ts = (j["a"], j.get("imp"), j.get("u"), j["aeff"], j["b"])
            _need_cuda(*ts)
            assert all(t is None or (t.is_contiguous() and t.dtype == torch.float32) for t in ts)
            k, v, _ = j["a"].shape
            vc = j["b"].shape[1]
            assert tuple(j["aeff"].shape) == (k, v, v) and tuple(j["b"].shape) == (k, vc, v)
            e = arr[q]
            e.a, e.imp, e.u, e.aeff, e.b = j["a"].data_ptr(), _ptr(j.get("imp")), _ptr(j.get("u")), j["aeff"].data_ptr(), j["b"].data_ptr()
            e.K, e.V, e.Vc = k, v, vc
        _check(lib.kg_gen_adj_prepare(arr, len(chunk), _stream()), "kg_gen_adj_prepare")


def gen_expand(y: Optional[torch.Tensor], A: Optional[torch.Tensor], U: Optional[torch.Tensor], rep: int, C_out: int,
               rs: Optional[torch.Tensor] = None, rbias: Optional[torch.Tensor] = None, B: Optional[torch.Tensor] = None):
    """Generator block, second half of the head (kg_gen_expand): y (N, K*C_out, Tc, Vc) = the gcn conv on the block's
    input grid, A (K, V, V) the effective adjacency, U (Vc, V) the up-sampling matrix (None: Vc == V), ``rep`` the
    frame repeat -> z (N, C_out, Tc*rep, V) = sum_k y_k (U A_k); rs (N, Cr, Tc, Vc) -> r (N, Cr, Tc*rep, V) =
    rs U + rbias.  Returns (z | None, r | None)."""
    lib = load_library()
    src = y if y is not None else rs
    if A is not None and not A.is_contiguous():
        A = A.contiguous()
    _need_cuda(y, A, U, rs, rbias, B)
    a = _GenArgs()
    n, _, tc, vc = src.shape
    v = U.shape[1] if U is not None else vc
    _gen_common(a, A, U, n, tc, vc, v, rep, B)
    z = r = None
    if y is not None:
        y = as_plane(y)
        k = A.shape[0] if A is not None else B.shape[0]
        assert y.shape[1] == k * C_out and (A is None or tuple(A.shape) == (k, v, v)), (y.shape, C_out)
        a.C, a.K = C_out, k
        _bind(a, "y", "y", y)
        z = _bind(a, "z", "z", new_plane(n, C_out, tc * rep, v, y.device))
        _count("kg_agg", 2.0 * k * vc * v * C_out * n * tc)
    if rs is not None:
        rs = as_plane(rs)
        assert tuple(rs.shape[2:]) == (tc, vc) and rs.shape[0] == n
        a.Cr = rs.shape[1]
        _bind(a, "rs", "rs", rs)
        a.rbias = _ptr(rbias)
        r = _bind(a, "r", "r", new_plane(n, rs.shape[1], tc * rep, v, rs.device))
        _count("kg_agg", 2.0 * vc * v * rs.shape[1] * n * tc)
    _check(lib.kg_gen_expand(C.byref(a), _stream()), "kg_gen_expand")
    return z, r


def gen_fold(gz: Optional[torch.Tensor], A: Optional[torch.Tensor], U: Optional[torch.Tensor], rep: int, K: int,
             gr: Optional[torch.Tensor] = None, want_zf: bool = False, y_out: Optional[torch.Tensor] = None,
             rs_out: Optional[torch.Tensor] = None, B: Optional[torch.Tensor] = None):
    """Adjoint of gen_expand (kg_gen_fold): gz (N, C, Tc*rep, V) -> gy (N, K*C, Tc, Vc) = fold(gz (U A_k)^T),
    gr (N, Cr, Tc*rep, V) -> grs (N, Cr, Tc, Vc) = fold(gr U^T), zf (N, C, Tc, V) = gz summed over the repeated frames
    (``want_zf``; gz itself when rep == 1).  ``y_out`` / ``rs_out``: plane tensors to write into (e.g. channel ranges
    of one (N, K*C + Cr, Tc, Vc) tensor).  Returns (gy | None, grs | None, zf | None)."""
    lib = load_library()
    src = gz if gz is not None else gr
    if A is not None and not A.is_contiguous():
        A = A.contiguous()
    _need_cuda(gz, A, U, gr, y_out, rs_out, B)
    n, _, tf, v = src.shape
    assert tf % rep == 0
    tc = tf // rep
    vc = U.shape[0] if U is not None else v
    a = _GenArgs()
    _gen_common(a, A, U, n, tc, vc, v, rep, B)
    gy = grs = zf = None
    if gz is not None:
        gz = as_plane(gz)
        c = gz.shape[1]
        a.C, a.K = c, K
        _bind(a, "z", "z", gz)
        gy = y_out if y_out is not None else new_plane(n, K * c, tc, vc, gz.device)
        assert tuple(gy.shape) == (n, K * c, tc, vc) and is_plane(gy)
        _bind(a, "y_out", "y", gy)
        if want_zf:
            zf = gz if rep == 1 else _bind(a, "zf", "zf", new_plane(n, c, tc, v, gz.device))
        _count("kg_agg", 2.0 * K * vc * v * c * n * tf)
    if gr is not None:
        gr = as_plane(gr)
        a.Cr = gr.shape[1]
        _bind(a, "r", "r", gr)
        grs = rs_out if rs_out is not None else new_plane(n, gr.shape[1], tc, vc, gr.device)
        assert tuple(grs.shape) == (n, gr.shape[1], tc, vc) and is_plane(grs)
        _bind(a, "rs_out", "rs", grs)
        _count("kg_agg", 2.0 * vc * v * gr.shape[1] * n * tf)
    _check(lib.kg_gen_fold(C.byref(a), _stream()), "kg_gen_fold")
    return gy, grs, zf


def gen_tail_bwd(g, out, act: int, u=None, bn_t=None, r=None, bn_r=None, noise=None, sinks=None, slope: float = 0.2,
                 coef: Optional[torch.Tensor] = None, stats_only: bool = False):
    """Backward of a generator block's tail out = act(BN_t(u) + BN_r(r) + w_noise noise) in two launches
    (kg_gen_tail_stats + kg_gen_tail_apply).  bn_t / bn_r: (gamma, mean, rstd) of the layer's training-mode BatchNorm or
    None; r without bn_r: identity residual.  ``sinks``: dict with optional contiguous (C,) tensors gamma_t, beta_t,
    gamma_r, beta_r, nw that RECEIVE (+=) the parameter gradients.  Returns (du, dr | None); du is dr's tensor when
    neither branch has BatchNorm (both equal g * act'(out)).
    ``coef``: the (6, C) tail coefficients when a fused backward launch of the NEXT block has computed them already
    (genblock_bwd: statistics launch and parameter-gradient adds skipped); ``stats_only``: only the statistics launch,
    returns the coefficients (the head of a fused backward chain)."""
    lib = load_library()
    g, out = as_plane(g), as_plane(out)
    n, c, t, v = g.shape
    sinks = sinks or {}
    a = _GenTailArgs()
    a.N, a.C, a.T, a.V, a.act, a.slope = n, c, t, v, act, slope
    _bind(a, "g", "g", g)
    _bind(a, "out", "o", out)
    keep = [g, out]
    if bn_t is not None:
        u = as_plane(u)
        gam, mean, rstd = (_vec(q, c, "gen_tail_bwd") for q in bn_t)
        _bind(a, "u", "u", u)
        a.gamma_t, a.mean_t, a.rstd_t = _ptr(gam), mean.data_ptr(), rstd.data_ptr()
        keep += [u, gam, mean, rstd]
    if r is not None:
        r = _bind(a, "r", "r", r, True)
        keep.append(r)
        if bn_r is not None:
            gam, mean, rstd = (_vec(q, c, "gen_tail_bwd") for q in bn_r)
            a.gamma_r, a.mean_r, a.rstd_r = _ptr(gam), mean.data_ptr(), rstd.data_ptr()
            keep += [gam, mean, rstd]
    if noise is not None:
        noise = noise.contiguous()
        a.noise = noise.data_ptr()
        keep.append(noise)
    _need_cuda(*keep, *sinks.values())
    for k_, t_ in sinks.items():
        if t_ is not None and (t_.numel() != c or not t_.is_contiguous()):
            raise ValueError("gen_tail_bwd: sink %s must be a contiguous (C,) tensor" % k_)
    a.dgamma_t, a.dbeta_t = _ptr(sinks.get("gamma_t")), _ptr(sinks.get("beta_t"))
    a.dgamma_r, a.dbeta_r, a.dnw = _ptr(sinks.get("gamma_r")), _ptr(sinks.get("beta_r")), _ptr(sinks.get("nw"))
    have_coef = coef is not None
    if have_coef:
        if tuple(coef.shape) != (6, c) or not coef.is_contiguous():
            raise ValueError("gen_tail_bwd: coef must be a contiguous (6, C) tensor")
        _need_cuda(coef)
    else:
        coef = torch.empty((6, c), dtype=torch.float32, device=g.device)
    a.coef = coef.data_ptr()
    if not have_coef:
        if c > SYNC_LEN:
            raise ValueError("gen_tail_bwd: %d channels exceed the %d ticket counters" % (c, SYNC_LEN))
        ws = _workspace("kg_gen_tail_workspace_bytes", a, g.device, tickets="counters")
        _check(lib.kg_gen_tail_stats(C.byref(a), _stream()), "kg_gen_tail_stats")
    if stats_only:
        return coef
    du = _bind(a, "du", "du", new_plane(n, c, t, v, g.device))
    dr = None
    if r is not None:
        dr = du if bn_t is None and bn_r is None else _bind(a, "dr", "dr", new_plane(n, c, t, v, g.device))
    _check(lib.kg_gen_tail_apply(C.byref(a), _stream()), "kg_gen_tail_apply")
    return du, dr


def gen_adj_finish(jobs: Sequence[dict]):
    """d edge_importance of several generator blocks in one launch (kg_gen_adj_finish).  Each job: dict(dbt (Kd, V, Vc)
    contiguous, u (Vc, V) | None, a (K, V, V) | None, out (K, V, V) contiguous view, accumulate)."""
    lib = load_library()
    for chunk in _chunks(jobs, GEN_ADJ_MAX_JOBS):
        arr = (_GenAdjJob * len(chunk))()
        for q, j in enumerate(chunk):
            dbt, out = j["dbt"], j["out"]
            _need_cuda(dbt, j.get("u"), j.get("a"), out)
            assert dbt.is_contiguous() and out.is_contiguous() and dbt.dim() == 3 and out.dim() == 3
            k, v, _ = out.shape
            kd, v2, vc = dbt.shape
            assert v2 == v and kd <= k, (dbt.shape, out.shape)
            e = arr[q]
            e.dbt, e.u, e.a, e.out = dbt.data_ptr(), _ptr(j.get("u")), _ptr(j.get("a")), out.data_ptr()
            e.K, e.Kd, e.V, e.Vc, e.accumulate = k, kd, v, vc, int(bool(j.get("accumulate", False)))
        _check(lib.kg_gen_adj_finish(arr, len(chunk), _stream()), "kg_gen_adj_finish")


# ---- fused generator block (kg_genblock.hip, ABI v9) -----------------------------------------------------------------

def _plane(t: Optional[torch.Tensor]) -> _Plane:
    p = _Plane()
    if t is not None:
        if not is_plane(t) or t.dtype != torch.float32:
            raise ValueError("genblock: plane tensor expected, got %s / strides %s" % (tuple(t.shape), t.stride()))
        p.p = t.data_ptr()
        p.sN, p.sC = _sn_sc(t)
    return p


class GenBlockDims(NamedTuple):
    """Static geometry of one generator block as the fused kernels take it (gen_trunk.GenBlockGeom)."""
    Cin: int
    C: int
    K: int
    Kp: int
    Tc: int
    Vc: int
    T: int
    V: int
    rep: int
    res_kind: int      # 0 none, 1 identity, 2 conv + BatchNorm
    bn_t: bool
    act: int


def _gb_common(a, d: GenBlockDims, slope):
    a.Cin, a.C, a.K, a.Kp, a.Tc, a.Vc, a.T, a.V, a.rep = d.Cin, d.C, d.K, d.Kp, d.Tc, d.Vc, d.T, d.V, d.rep
    a.res_kind, a.bn_t, a.act, a.slope = d.res_kind, int(d.bn_t), d.act, slope


def _gb_weights(a, wg, wr, wt, B, U):
    for t in (wg, wr, wt, B, U):
        if t is not None and (not t.is_contiguous() or t.dtype != torch.float32):
            raise ValueError("genblock: weights / adjacency must be contiguous fp32")
    a.wg, a.wr, a.wt, a.b, a.u = wg.data_ptr(), _ptr(wr), wt.data_ptr(), B.data_ptr(), _ptr(U)


def genblock_supported(d: GenBlockDims, n: int, wg, wr, wt, backward: bool = False) -> bool:
    """Can the fused kernels run this block (per-sample working set in LDS, contraction shapes, 16-byte aligned weight
    rows)?  Otherwise the staged entry points apply."""
    lib = load_library()
    if backward:
        a = _GenBlockBwdArgs()
        a.N = n
        _gb_common(a, d, 0.2)
        return lib.kg_genblock_bwd_lds_bytes(C.byref(a)) >= 0
    a = _GenBlockArgs()
    a.N, a.groups = n, 1
    _gb_common(a, d, 0.2)
    a.wg, a.wr, a.wt = wg.data_ptr(), _ptr(wr), wt.data_ptr()
    return lib.kg_genblock_lds_bytes(C.byref(a)) >= 0


last_genblock_form = None  # set to a list: genblock_fwd / genblock_bwd / genblock_infer append the form (genblock_form: a dict)
                           # of every launch, in call order - as last_conv_form


def genblock_form(d: GenBlockDims, n: int, direction: str = "fwd", *, groups: int = 1, prev: bool = False,
                  wg_aligned: bool = True, wr_aligned: bool = True, wt_aligned: bool = True) -> dict:
    """kg_genblock_form: the instantiation (``geometry``: index into the compile-time geometries, -1 = the run-time form),
    the path of the two contractions (mfma0 / mfma1, VALU row buckets mv0 / mv1), the dynamic LDS (-1: refused) and the grid
    of a ``direction`` ("fwd" / "bwd" / "infer") launch under the current KG_GB_RT switch.  Host code only: no GPU."""
    q = _GenBlockFormQuery()
    q.N, q.groups = n, groups
    q.Cin, q.C, q.K, q.Kp, q.Tc, q.Vc, q.T, q.V, q.rep = d.Cin, d.C, d.K, d.Kp, d.Tc, d.Vc, d.T, d.V, d.rep
    q.res_kind, q.bn_t = d.res_kind, int(d.bn_t)
    q.dir = {"fwd": GB_DIR_FWD, "bwd": GB_DIR_BWD, "infer": GB_DIR_INFER}[direction]
    q.prev, q.wg_aligned, q.wr_aligned, q.wt_aligned = int(prev), int(wg_aligned), int(wr_aligned), int(wt_aligned)
    f = _GenBlockForm()
    _check(load_library().kg_genblock_form(C.byref(q), C.byref(f)), "kg_genblock_form")
    out = {k: getattr(f, k) for k, *_ in _GenBlockForm._fields_}
    out["dir"] = direction
    return out


def _gb_record_form(d: GenBlockDims, n: int, direction: str, a, groups: int = 1, prev: bool = False):
    if last_genblock_form is not None:
        al = lambda p: p is None or p % 16 == 0
        last_genblock_form.append(genblock_form(d, n, direction, groups=groups, prev=prev, wg_aligned=al(a.wg), wr_aligned=al(a.wr),
                                                wt_aligned=al(a.wt)))


def _gb_bn(layer: _GenBnLayer, bn: dict, c: int, groups: int, device):
    vecs = [_vec(bn.get(k), c, "genblock_fwd") for k in ("gamma", "beta", "running_mean", "running_var")]
    nbt = bn.get("num_batches_tracked")
    _need_cuda(*vecs, nbt)
    layer.gamma, layer.beta, layer.running_mean, layer.running_var = [_ptr(q) for q in vecs]
    if nbt is not None:
        assert nbt.dtype == torch.int64
        layer.num_batches_tracked = nbt.data_ptr()
    layer.momentum, layer.eps = float(bn["momentum"]), float(bn["eps"])
    coef = torch.empty((groups, 4, c), dtype=torch.float32, device=device)
    layer.coef = coef.data_ptr()
    return coef


def genblock_fwd(d: GenBlockDims, *, x=None, pend=None, wg, wr=None, br=None, wt, bt=None, B, U=None, bn_t=None, bn_r=None,
                 groups: int = 1, noise=None, nw=None, slope: float = 0.2) -> dict:
    """One generator block forward in ONE launch (kg_genblock_fwd).  ``x`` (N, Cin, Tc, Vc): finished input, or ``pend`` =
    dict(u, r | None, ct | None, cr | None, noise | None, nw | None, act): the previous block's pending tail
    act(u * ct.scale + ct.shift + r * cr.scale + cr.shift + nw * noise) with ct / cr its (groups, 4, Cin) BatchNorm
    coefficients - applied here, the result written to the returned ``x``.  bn_t / bn_r: dict(gamma, beta, running_mean,
    running_var, num_batches_tracked, momentum, eps) of the block's training-mode BatchNorm layers.  A block without any
    BatchNorm finishes itself with ``noise`` / ``nw`` (returned ``out``).  Returns dict(x, yc, z, r, u, ct, cr, out)."""
    lib = load_library()
    a = _GenBlockArgs()
    _gb_common(a, d, slope)
    if (bn_t is not None) != bool(d.bn_t) or (bn_r is not None) != (d.res_kind == 2):
        raise ValueError("genblock_fwd: BatchNorm layers do not match the block's geometry")
    keep = []
    if x is not None:
        x = as_plane(x)
        n = x.shape[0]
        a.x = _plane(x)
        dev = x.device
        if tuple(x.shape[1:]) != (d.Cin, d.Tc, d.Vc):
            raise ValueError("genblock_fwd: input %s does not match (%d, %d, %d)" % (tuple(x.shape), d.Cin, d.Tc, d.Vc))
    else:
        pu = as_plane(pend["u"])
        n, dev = pu.shape[0], pu.device
        if tuple(pu.shape[1:]) != (d.Cin, d.Tc, d.Vc):
            raise ValueError("genblock_fwd: pending tail %s does not match (%d, %d, %d)" % (tuple(pu.shape), d.Cin, d.Tc, d.Vc))
        a.pu = _plane(pu)
        pr = pend.get("r")
        if pr is not None:
            pr = as_plane(pr)
            a.pr = _plane(pr)
        for key, fld in (("ct", "pcoef_t"), ("cr", "pcoef_r")):
            cf = pend.get(key)
            if cf is not None:
                if tuple(cf.shape) != (groups, 4, d.Cin) or not cf.is_contiguous():
                    raise ValueError("genblock_fwd: pending %s must be a contiguous (groups, 4, Cin) tensor" % key)
                setattr(a, fld, cf.data_ptr())
        pn, pw = pend.get("noise"), pend.get("nw")
        if pn is not None and pw is not None:
            pn, pw = pn.contiguous(), pw.reshape(-1).contiguous()
            a.pnoise, a.pnw = pn.data_ptr(), pw.data_ptr()
        a.pact = int(pend["act"])
        x = new_plane(n, d.Cin, d.Tc, d.Vc, dev)
        a.xout = _plane(x)
        keep += [pu, pr, pn, pw, pend.get("ct"), pend.get("cr")]
        _need_cuda(*keep)
    a.N, a.groups = n, groups
    _gb_weights(a, wg, wr, wt, B, U)
    a.br, a.bt = _ptr(br), _ptr(bt)
    _need_cuda(x, wg, wr, br, wt, bt, B, U, noise, nw)
    Mh = d.Kp * d.C + (d.C if d.res_kind == 2 else 0)
    yc = new_plane(n, Mh, d.Tc, d.Vc, dev)
    z = new_plane(n, d.C, d.T, d.V, dev)
    u = new_plane(n, d.C, d.T, d.V, dev)
    r = new_plane(n, d.C, d.T, d.V, dev) if d.res_kind != 0 else None
    a.yc, a.z, a.uo, a.r = _plane(yc), _plane(z), _plane(u), _plane(r)
    ct = _gb_bn(a.bt_, bn_t, d.C, groups, dev) if bn_t is not None else None
    cr = _gb_bn(a.br_, bn_r, d.C, groups, dev) if bn_r is not None else None
    out = None
    if ct is None and cr is None:
        out = new_plane(n, d.C, d.T, d.V, dev)
        a.out = _plane(out)
        if noise is not None and nw is not None:
            noise, nw = noise.contiguous(), nw.reshape(-1).contiguous()
            a.noise, a.nw = noise.data_ptr(), nw.data_ptr()
    else:
        ws = _workspace("kg_genblock_workspace_bytes", a, dev, tickets="counters")
    _count("kg_genblock", 2.0 * n * (Mh * d.Cin * d.Tc * d.Vc + 3 * d.C * d.C * d.T * d.V) +
           2.0 * n * (d.Kp + (1 if d.res_kind else 0)) * d.Vc * d.V * d.C * d.Tc)
    _gb_record_form(d, n, "fwd", a, groups=groups)
    _check(lib.kg_genblock_fwd(C.byref(a), _stream()), "kg_genblock_fwd")
    return dict(x=x, yc=yc, z=z, r=r, u=u, ct=ct, cr=cr, out=out)


def genblock_bwd(d: GenBlockDims, *, g, out, u=None, r=None, coef, wg, wr=None, wt, B, U=None, prev=None, slope: float = 0.2) -> dict:
    """One generator block backward in ONE launch (kg_genblock_bwd): g = d loss / d out, (out, u, r) the block's tape,
    coef (6, C) its tail coefficients (gen_tail_bwd(stats_only=True) or the previous call's ``pcoef``).  ``prev`` =
    dict(x, u | None, r | None, noise | None, act, bn_t = (gamma, mean, rstd) | None, bn_r likewise, sinks = dict of (Cin,)
    tensors gamma_t, beta_t, gamma_r, beta_r, nw that RECEIVE the parameter gradients): the block before this one, whose
    tail statistics are taken on the way out (returned ``pcoef`` (6, Cin)).  Returns dict(du, dr, gyc, zf, gx, pcoef);
    dr is du when the block has a residual but no BatchNorm at all."""
    lib = load_library()
    a = _GenBlockBwdArgs()
    _gb_common(a, d, slope)
    g, out = as_plane(g), as_plane(out)
    n, dev = g.shape[0], g.device
    a.N = n
    a.g, a.out = _plane(g), _plane(out)
    keep = [g, out, coef]
    if d.bn_t:
        u = as_plane(u)
        a.uo = _plane(u)
        keep.append(u)
    if d.res_kind == 2:
        r = as_plane(r)
        a.r = _plane(r)
        keep.append(r)
    if tuple(coef.shape) != (6, d.C) or not coef.is_contiguous():
        raise ValueError("genblock_bwd: coef must be a contiguous (6, C) tensor")
    a.coef = coef.data_ptr()
    _gb_weights(a, wg, wr, wt, B, U)
    _need_cuda(*keep, wg, wr, wt, B, U)
    Mh = d.Kp * d.C + (d.C if d.res_kind == 2 else 0)
    du = new_plane(n, d.C, d.T, d.V, dev)
    dr = None
    if d.res_kind == 2 or (d.res_kind == 1 and d.bn_t):
        dr = new_plane(n, d.C, d.T, d.V, dev)
    gyc = new_plane(n, Mh, d.Tc, d.Vc, dev)
    zf = new_plane(n, d.C, d.Tc, d.V, dev)
    gx = new_plane(n, d.Cin, d.Tc, d.Vc, dev)
    a.du, a.dr, a.gyc, a.zf, a.gx = _plane(du), _plane(dr), _plane(gyc), _plane(zf), _plane(gx)
    pcoef = None
    if prev is not None:
        px = as_plane(prev["x"])
        a.px = _plane(px)
        a.pact = int(prev["act"])
        sinks = prev.get("sinks") or {}
        keep2 = [px]
        if prev.get("bn_t") is not None:
            pu = as_plane(prev["u"])
            gam, mean, rstd = (_vec(q, d.Cin, "genblock_bwd") for q in prev["bn_t"])
            a.pu = _plane(pu)
            a.pgamma_t, a.pmean_t, a.prstd_t = _ptr(gam), mean.data_ptr(), rstd.data_ptr()
            keep2 += [pu, gam, mean, rstd]
        if prev.get("bn_r") is not None:
            pr = as_plane(prev["r"])
            gam, mean, rstd = (_vec(q, d.Cin, "genblock_bwd") for q in prev["bn_r"])
            a.pr = _plane(pr)
            a.pgamma_r, a.pmean_r, a.prstd_r = _ptr(gam), mean.data_ptr(), rstd.data_ptr()
            keep2 += [pr, gam, mean, rstd]
        pn = prev.get("noise")
        if pn is not None:
            pn = pn.contiguous()
            a.pnoise = pn.data_ptr()
            keep2.append(pn)
        for k_, t_ in sinks.items():
            if t_ is not None and (t_.numel() != d.Cin or not t_.is_contiguous()):
                raise ValueError("genblock_bwd: sink %s must be a contiguous (Cin,) tensor" % k_)
        _need_cuda(*keep2, *sinks.values())
        a.dgamma_t, a.dbeta_t = _ptr(sinks.get("gamma_t")), _ptr(sinks.get("beta_t"))
        a.dgamma_r, a.dbeta_r, a.dnw = _ptr(sinks.get("gamma_r")), _ptr(sinks.get("beta_r")), _ptr(sinks.get("nw"))
        pcoef = torch.empty((6, d.Cin), dtype=torch.float32, device=dev)
        a.pcoef = pcoef.data_ptr()
        ws = _workspace("kg_genblock_bwd_workspace_bytes", a, dev, tickets="counters")
    _count("kg_genblock", 2.0 * n * (Mh * d.Cin * d.Tc * d.Vc + 3 * d.C * d.C * d.T * d.V) +
           2.0 * n * (d.Kp + (1 if d.res_kind else 0)) * d.Vc * d.V * d.C * d.T)
    _gb_record_form(d, n, "bwd", a, prev=prev is not None)
    _check(lib.kg_genblock_bwd(C.byref(a), _stream()), "kg_genblock_bwd")
    if dr is None and d.res_kind != 0:
        dr = du
    return dict(du=du, dr=dr, gyc=gyc, zf=zf, gx=gx, pcoef=pcoef)


def _rowsum_fill(a, x, y, want_second: int, out, out2, accumulate: int):
    """Fill one KgRowsumArgs (without shift and workspace) from the plane tensor x; returns the tensors it bound."""
    n, c, t, v = x.shape
    a.N, a.C, a.T, a.V = n, c, t, v
    _bind(a, "x", "x", x)
    if y is not None:
        if y.shape[1] == 1 and c > 1:          # one plane for all channels: channel stride 0
            y = y.contiguous()
            a.y, a.y_sN, a.y_sC = y.data_ptr(), t * v, 0
        else:
            y = _bind(a, "y", "y", y, True)
    a.want_second = want_second      # 1: both rows; 2: the product row alone
    a.out, a.out2, a.accumulate = out.data_ptr(), _ptr(out2), accumulate
    return x, y


def rowsum(x: torch.Tensor, y: Optional[torch.Tensor] = None, second: bool = False,
           shift: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
           accumulate: bool = False, out2: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(1|2, C): sum over (n,t,v) of x, and of x*(y-shift) ((x-shift)^2 when y is None).  y may
    broadcast over C (shape (N,1,T,V)); shift is per channel.  out / accumulate as in wgrad; out2: a second
    destination for the same sums."""
    lib = load_library()
    x = as_plane(x)
    _need_cuda(x, y, shift)
    c = x.shape[1]
    a = _RowsumArgs()
    if shift is not None:
        shift = shift.reshape(-1).contiguous()
        a.shift = shift.data_ptr()
    rows = 2 if int(second) == 1 else 1
    if out is None:
        if accumulate:
            raise ValueError("rowsum: accumulate needs out")
        out = torch.empty((rows, c), dtype=torch.float32, device=x.device)
    else:
        _need_cuda(_dest(out, rows * c, "rowsum: out must be a contiguous fp32 tensor of %d elements" % (rows * c)))
    if out2 is not None:
        _need_cuda(_dest(out2, rows * c, "rowsum: out2 must be a contiguous fp32 tensor of %d elements" % (rows * c)))
    held = _rowsum_fill(a, x, y, int(second), out, out2, int(accumulate))
    ws = _workspace("kg_rowsum_workspace_bytes", a, x.device)
    _check(lib.kg_rowsum(C.byref(a), _stream()), "kg_rowsum")
    return out


def rowsum_many(jobs: Sequence[dict]):
    """Per-channel sums over (n, t, v) of several tensors in one launch (+ one finishing launch): each job
    dict(x, out, out2=None, accumulate=False) writes / adds sum(x) per channel to `out` (and `out2`); with ``y``
    (same shape as x, or (N,1,T,V)) the sums are of x*y instead."""
    lib = load_library()
    if not jobs:
        return
    arr = (_RowsumArgs * len(jobs))()
    held = []                # the tensors every job bound (converted copies among them), until the launch is enqueued
    for i, j in enumerate(jobs):
        x = as_plane(j["x"])
        out, out2, y = j["out"], j.get("out2"), j.get("y")
        _need_cuda(x, out, out2)
        for o in (out, out2):
            if o is not None:
                _dest(o, x.shape[1], "rowsum_many: destinations must be contiguous fp32 vectors of C elements")
        _need_cuda(y)
        held.append(_rowsum_fill(arr[i], x, y, 0 if y is None else 2, out, out2, int(bool(j.get("accumulate", False)))))
    ws = _workspace("kg_rowsum_many_workspace_bytes", arr, jobs[0]["x"].device, len(jobs))
    _check(lib.kg_rowsum_many(arr, len(jobs), ws.data_ptr(), ws.numel() * 4, _stream()), "kg_rowsum_many")


def _elt_args(x, out, act, slope):
    a = _EltArgs()
    a.N, a.C, a.T, a.V = x.shape
    _bind(a, "x", "x", x)
    _bind(a, "out", "o", out)
    a.act, a.slope = act, slope
    return a


def act_bwd(g: torch.Tensor, ref: torch.Tensor, act: int, slope: float = 0.2) -> torch.Tensor:
    lib = load_library()
    g = as_plane(g)
    ref = as_plane(ref)
    _need_cuda(g, ref)
    out = new_plane(*g.shape, g.device)
    a = _elt_args(g, out, act, slope)
    _bind(a, "r", "r", ref)
    _check(lib.kg_act_bwd(C.byref(a), _stream()), "kg_act_bwd")
    return out


def affine_act(x, sx=None, bx=None, r=None, sr=None, br=None, noise=None, nw=None,
               act: int = ACT_NONE, slope: float = 0.2, out: Optional[torch.Tensor] = None,
               groups: int = 1, coef_gs: int = 0) -> torch.Tensor:
    """``out``: optional plane tensor of x's shape to write into (e.g. a sample range of a larger buffer).
    ``groups`` > 1: x holds that many batches stacked along N; sx / bx / sr / br are the FIRST batch's vectors inside a
    buffer that holds batch q's at + q * coef_gs floats (the (groups, 4, C) result of bn_fwd_many: coef_gs = 4 C)."""
    lib = load_library()
    x = as_plane(x)
    vecs = [None if t is None else t.reshape(-1).contiguous() for t in (sx, bx, sr, br, nw)]
    _need_cuda(x, r, noise, out, *vecs)
    if out is None:
        out = new_plane(*x.shape, x.device)
    elif tuple(out.shape) != tuple(x.shape) or not is_plane(out) or out.dtype != torch.float32:
        raise ValueError("affine_act: out must be a plane tensor of x's shape")
    a = _elt_args(x, out, act, slope)
    if r is not None:
        r = _bind(a, "r", "r", r, True)
    if noise is not None:
        noise = noise.contiguous()
        a.noise = noise.data_ptr()
    a.sx, a.bx, a.sr, a.br, a.nw = [_ptr(t) for t in vecs]
    a.groups, a.coef_gs = int(groups), int(coef_gs)
    _check(lib.kg_affine_act(C.byref(a), _stream()), "kg_affine_act")
    return out


def _gp_args(g):
    """KgGpArgs of the per-sample gradients g (a plane tensor)"""
    a = _GpArgs()
    a.N, a.C, a.T, a.V = g.shape
    _bind(a, "g", "g", g)
    return a


def gp_fwd(g: torch.Tensor):
    """(nrm (N,), gp ()) of the WGAN-GP penalty for per-sample gradients g (N, C, T, V): kg_gp_fwd"""
    lib = load_library()
    g = as_plane(g)
    _need_cuda(g)
    a = _gp_args(g)
    nrm = torch.empty(g.shape[0], dtype=torch.float32, device=g.device)
    gp = torch.empty((), dtype=torch.float32, device=g.device)
    a.nrm, a.gp = nrm.data_ptr(), gp.data_ptr()
    _check(lib.kg_gp_fwd(C.byref(a), _stream()), "kg_gp_fwd")
    return nrm, gp


def gp_bwd(g: torch.Tensor, nrm: torch.Tensor, gout: torch.Tensor) -> torch.Tensor:
    """d gp / d g * gout (gout: 0-dim device tensor): kg_gp_bwd"""
    lib = load_library()
    g = as_plane(g)
    gout = gout.reshape(1).contiguous()
    _need_cuda(g, nrm, gout)
    a = _gp_args(g)
    a.nrm, a.gout = nrm.data_ptr(), gout.data_ptr()
    out = _bind(a, "out", "o", new_plane(*g.shape, g.device))
    _check(lib.kg_gp_bwd(C.byref(a), _stream()), "kg_gp_bwd")
    return out


def _vec(t: Optional[torch.Tensor], c: int, what: str):
    return None if t is None else _dest(t, c, f"{what}: expected a contiguous fp32 vector of {c} elements")


def _bn_fwd_fill(a, who: str, x, gamma, beta, running_mean, running_var, nbt, momentum, eps, training, groups: Optional[int] = None):
    """Fill one KgBnArgs for the forward statistics of the plane tensor x (``groups`` batches stacked along N; None: the
    single form, whose coefficients are (4, C)); returns the coefficient tensor it allocated."""
    n, c, t, v = x.shape
    vecs = [_vec(q, c, who) for q in (gamma, beta, running_mean, running_var)]
    _need_cuda(x, *vecs, nbt)
    a.N, a.C, a.T, a.V = n // (groups or 1), c, t, v
    _bind(a, "x", "x", x)
    a.gamma, a.beta, a.running_mean, a.running_var = [_ptr(q) for q in vecs]
    if nbt is not None:
        assert nbt.dtype == torch.int64
        a.num_batches_tracked = nbt.data_ptr()
    a.momentum, a.eps, a.training = float(momentum), float(eps), int(bool(training))
    coef = torch.empty((4, c) if groups is None else (groups, 4, c), dtype=torch.float32, device=x.device)
    a.coef = coef.data_ptr()
    return coef


def bn_fwd(x: torch.Tensor, gamma, beta, running_mean, running_var, num_batches_tracked, training: bool,
           momentum: float, eps: float) -> torch.Tensor:
    """BatchNorm2d statistics of x and the per-channel coefficients, one launch: returns (4, C) =
    [scale, shift, mean, rstd]; training mode updates the running statistics in place (torch semantics)."""
    lib = load_library()
    x = as_plane(x)
    a = _BnArgs()
    coef = _bn_fwd_fill(a, "bn_fwd", x, gamma, beta, running_mean, running_var, num_batches_tracked, momentum, eps, training)
    _check(lib.kg_bn_fwd(C.byref(a), _stream()), "kg_bn_fwd")
    return coef


def _bn_many(who: str, arr, coefs):
    """the shared end of bn_fwd_many / bn_bwd_many: ticket-counter limit, scratch and the launch of lib.kg_<who>"""
    total_c = sum(cf.shape[-1] for cf in coefs)
    if total_c > SYNC_LEN:
        raise ValueError("%s: %d channels exceed the %d ticket counters" % (who, total_c, SYNC_LEN))
    ws = _workspace("kg_%s_workspace_bytes" % who, arr, coefs[0].device if coefs else None, len(arr))   # (no jobs: its message)
    sync = _sync_buffer(coefs[0].device)
    _check(getattr(load_library(), "kg_" + who)(arr, len(arr), ws.data_ptr(), ws.numel() * 4, sync.data_ptr(), sync.numel(),
                                               _stream()), "kg_" + who)
    return coefs


def bn_fwd_many(jobs: Sequence[dict]):
    """Training-mode BatchNorm2d statistics of up to four layers in ONE launch.  Each job: dict(x, gamma, beta,
    running_mean, running_var, num_batches_tracked, momentum, eps, groups): x holds ``groups`` independent batches
    stacked along N; returns one (groups, 4, C) tensor [scale, shift, mean, rstd] per job, the running statistics
    updated batch by batch as ``groups`` bn_fwd calls would."""
    arr = (_BnJob * len(jobs))()
    xs, coefs = [], []          # xs: the (converted) inputs, held until the launch is enqueued
    for i, j in enumerate(jobs):
        x = as_plane(j["x"])
        groups = int(j.get("groups", 1))
        if x.shape[0] % groups:
            raise ValueError("bn_fwd_many: N=%d is not a multiple of groups=%d" % (x.shape[0], groups))
        coefs.append(_bn_fwd_fill(arr[i].a, "bn_fwd_many", x, j.get("gamma"), j.get("beta"), j.get("running_mean"),
                                  j.get("running_var"), j.get("num_batches_tracked"), j["momentum"], j["eps"], True, groups))
        arr[i].groups = groups
        xs.append(x)
    return _bn_many("bn_fwd_many", arr, coefs)


def _bn_bwd_fill(a, who: str, g, x, gamma, mean, rstd, training):
    """Fill one KgBnArgs for the backward coefficients; returns ((5, C) coefficient tensor, the tensors it bound)."""
    g, x = as_plane(g), as_plane(x)
    n, c, t, v = x.shape
    gamma, mean, rstd = _vec(gamma, c, who), _vec(mean, c, who), _vec(rstd, c, who)
    _need_cuda(g, x, gamma, mean, rstd)
    a.N, a.C, a.T, a.V = n, c, t, v
    _bind(a, "x", "x", x)
    _bind(a, "g", "g", g)
    a.gamma, a.mean, a.rstd = _ptr(gamma), _ptr(mean), _ptr(rstd)
    a.training = int(bool(training))
    coef = torch.empty((5, c), dtype=torch.float32, device=x.device)
    a.coef = coef.data_ptr()
    return coef, (g, x)


def bn_bwd(g: torch.Tensor, x: torch.Tensor, gamma, mean: torch.Tensor, rstd: torch.Tensor, training: bool) -> torch.Tensor:
    """(5, C) = [a, b, c, dgamma, dbeta] of the BatchNorm2d backward (dL/dx = a*g + b*x + c), one launch."""
    lib = load_library()
    a = _BnArgs()
    coef, held = _bn_bwd_fill(a, "bn_bwd", g, x, gamma, mean, rstd, training)
    _check(lib.kg_bn_bwd(C.byref(a), _stream()), "kg_bn_bwd")
    return coef


def bn_bwd_many(jobs: Sequence[dict]):
    """bn_bwd of up to four layers in ONE launch (chunked partial sums, many workgroups per channel): each job
    dict(g, x, gamma, mean, rstd, training) -> its (5, C) coefficients [a, b, c, dgamma, dbeta]."""
    arr = (_BnArgs * len(jobs))()
    # (every job's coefficients and the tensors it bound, the latter held until the launch is enqueued)
    filled = [_bn_bwd_fill(arr[i], "bn_bwd_many", j["g"], j["x"], j.get("gamma"), j["mean"], j["rstd"], j["training"])
              for i, j in enumerate(jobs)]
    return _bn_many("bn_bwd_many", arr, [coef for coef, _ in filled])


def adam_step(p, g, m, v, lr, b1, b2, eps, step_t: torch.Tensor, grad_scale: float = 1.0, zero_grad: bool = False):
    """Flat-buffer Adam; ``step_t`` holds the 1-based number of THIS step (the caller has incremented it).  ``zero_grad``
    (kg_adam_step_fused): the launch also clears the gradient it has consumed."""
    lib = load_library()
    _need_cuda(p, g, m, v, step_t)
    assert p.is_contiguous() and g.is_contiguous() and m.is_contiguous() and v.is_contiguous()
    assert step_t.dtype == torch.int32
    if zero_grad:
        _check(lib.kg_adam_step_fused(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), lr, b1, b2, eps,
                                      step_t.data_ptr(), grad_scale, 1, _stream()), "kg_adam_step_fused")
        return
    _check(lib.kg_adam_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(),
                            lr, b1, b2, eps, step_t.data_ptr(), grad_scale, _stream()), "kg_adam_step")


def adam_step_ema(p, g, m, v, e, lr, b1, b2, eps, step_t: torch.Tensor, grad_scale: float, zero_grad: bool, decay: float,
                  warmup: float):
    """``adam_step`` with the parameters' moving average ``e`` updated by the same launch (kg_adam_step_ema):
    e += (1 - beta_s) (p_new - e), beta_s = decay, or min(decay, (1 + s) / (warmup + s)) with s = step_t when warmup != 0."""
    lib = load_library()
    _need_cuda(p, g, m, v, e, step_t)
    assert p.is_contiguous() and g.is_contiguous() and m.is_contiguous() and v.is_contiguous() and e.is_contiguous()
    assert g.numel() == m.numel() == v.numel() == e.numel() == p.numel() and e.dtype == torch.float32
    assert step_t.dtype == torch.int32
    _check(lib.kg_adam_step_ema(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), e.data_ptr(), p.numel(), lr, b1, b2, eps,
                                step_t.data_ptr(), grad_scale, 1 if zero_grad else 0, decay, warmup, _stream()),
           "kg_adam_step_ema")


# ---- container-level fusions around the discriminator's blocks (kg_disc.hip) ---------------------------------------------

def _head_args(h, w=None, gv=None):
    """KgHeadArgs with the operands the three head entry points share: h (N, C, T, V), the Linear weight w (C values) and the
    per-sample gradient gv (N values, flat); returns (args, h as bound)."""
    a = _HeadArgs()
    h = _bind(a, "h", "h", h, True)
    a.N, a.C, a.T, a.V = h.shape
    if w is not None:
        w = w.reshape(-1)
        assert w.is_contiguous() and w.numel() == h.shape[1]
        a.w = w.data_ptr()
    if gv is not None:
        assert gv.numel() == h.shape[0]
        a.gv = gv.data_ptr()
    return a, h


def head_fwd(h: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor]) -> torch.Tensor:
    """v (N,) = b + mean_{t,v}(h) @ w: global average pool + Linear(latent, 1) (kg_head_fwd)"""
    lib = load_library()
    _need_cuda(h, w, b)
    a, h = _head_args(h, w)
    a.b = _ptr(b)
    v = torch.empty(h.shape[0], dtype=torch.float32, device=h.device)
    a.v = v.data_ptr()
    _check(lib.kg_head_fwd(C.byref(a), _stream()), "kg_head_fwd")
    return v


def head_bwd(gv: torch.Tensor, w: torch.Tensor, h: torch.Tensor, masked: bool = True, slope: float = 0.2) -> torch.Tensor:
    """(N, C, T, V) top gradient gv[n] w[c] / (T V), times lrelu'(h) when ``masked`` (kg_head_bwd)"""
    lib = load_library()
    gv = gv.reshape(-1).contiguous()
    _need_cuda(gv, w, h)
    a, h = _head_args(h, w, gv)
    a.masked, a.slope = int(bool(masked)), slope
    g = _bind(a, "g", "g", new_plane(*h.shape, h.device))
    _check(lib.kg_head_bwd(C.byref(a), _stream()), "kg_head_bwd")
    return g


def head_wgrad(x: torch.Tensor, gv: torch.Tensor, dw: torch.Tensor, db: Optional[torch.Tensor], accumulate: bool = True):
    """dw (C,) (+)= sum_n gv[n] mean_{t,v} x[n]; db (1,) (+)= sum_n gv[n] (kg_head_wgrad)"""
    lib = load_library()
    gv = gv.reshape(-1).contiguous()
    _need_cuda(x, gv, dw, db)
    a, x = _head_args(x, None, gv)
    assert dw.is_contiguous() and dw.numel() == x.shape[1] and (db is None or db.numel() == 1)
    a.dw, a.db, a.accumulate = dw.data_ptr(), _ptr(db), int(bool(accumulate))
    _check(lib.kg_head_wgrad(C.byref(a), _stream()), "kg_head_wgrad")


# ---- the action classifier's head (kg_cls.hip; classifier.Classifier) -----------------------------------------------------

def _cls_head_args(n: int, c: int, t: int, v: int, f: int, l: int, slope: float = 0.2) -> _ClsHeadArgs:
    a = _ClsHeadArgs()
    a.N, a.C, a.T, a.V, a.F, a.L, a.slope = int(n), int(c), int(t), int(v), int(f), int(l), float(slope)
    return a


def _cls_flat(t: torch.Tensor, n: int, dtype, what: str) -> torch.Tensor:
    if t.numel() != n or not t.is_contiguous() or t.dtype != dtype:
        raise ValueError(f"kg_cls_head: {what} must be contiguous {dtype} of {n} elements")
    return t


def cls_head_workspace_bytes(n: int, c: int, t: int, v: int, f: int, l: int) -> int:
    """bytes of the scratch kg_cls_head_bwd fills and kg_cls_head_wgrad reads: 4 N (L + F)"""
    return _query("kg_cls_head_workspace_bytes", _cls_head_args(n, c, t, v, f, l))


def cls_head_fwd(h: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor,
                 labels: Optional[torch.Tensor] = None, slope: float = 0.2, feat_out: Optional[torch.Tensor] = None,
                 pred_out: Optional[torch.Tensor] = None) -> dict:
    """Global average pool -> fc1 + LeakyReLU -> fcn -> argmax and, with ``labels`` (N,) int64, the softmax cross-entropy
    (kg_cls_head_fwd; no host synchronisation).  Returns dict(pooled (N, C), feat (N, F), logits (N, L), pred (N,) int32) and
    with labels loss_per_sample (N,), loss (0-d), correct (0-d int32); else those three are None.  ``feat_out`` (N, F) fp32 /
    ``pred_out`` (N,) int32: contiguous row slices of larger (N_total, F) / (N_total,) buffers that the launch writes - and
    the dict returns - instead of fresh tensors: the chunks of a large set land in one feature matrix."""
    lib = load_library()
    _need_cuda(h, w1, b1, w2, b2, labels, feat_out, pred_out)
    f, l = w1.shape[0], w2.shape[0]
    a = _cls_head_args(*h.shape, f, l, slope)
    h = _bind(a, "h", "h", h, True)
    n, c = h.shape[0], h.shape[1]
    a.w1, a.b1 = _cls_flat(w1, f * c, torch.float32, "w1").data_ptr(), _cls_flat(b1, f, torch.float32, "b1").data_ptr()
    a.w2, a.b2 = _cls_flat(w2, l * f, torch.float32, "w2").data_ptr(), _cls_flat(b2, l, torch.float32, "b2").data_ptr()
    dev = h.device
    if feat_out is not None and tuple(feat_out.shape) != (n, f):
        raise ValueError(f"kg_cls_head: feat_out must be ({n}, {f}), got {tuple(feat_out.shape)}")
    if pred_out is not None and tuple(pred_out.shape) != (n,):
        raise ValueError(f"kg_cls_head: pred_out must be ({n},), got {tuple(pred_out.shape)}")
    out = dict(pooled=torch.empty((n, c), dtype=torch.float32, device=dev),
               feat=torch.empty((n, f), dtype=torch.float32, device=dev) if feat_out is None
               else _cls_flat(feat_out, n * f, torch.float32, "feat_out"),
               logits=torch.empty((n, l), dtype=torch.float32, device=dev),
               pred=torch.empty(n, dtype=torch.int32, device=dev) if pred_out is None
               else _cls_flat(pred_out, n, torch.int32, "pred_out"),
               loss_per_sample=None, loss=None, correct=None)
    a.pooled, a.feat, a.logits, a.pred = (out[k].data_ptr() for k in ("pooled", "feat", "logits", "pred"))
    if labels is not None:
        a.labels = _cls_flat(labels, n, torch.int64, "labels").data_ptr()
        out["loss_per_sample"] = torch.empty(n, dtype=torch.float32, device=dev)
        out["loss"] = torch.empty((), dtype=torch.float32, device=dev)
        out["correct"] = torch.empty((), dtype=torch.int32, device=dev)
        a.loss_per_sample, a.loss, a.correct = (out[k].data_ptr() for k in ("loss_per_sample", "loss", "correct"))
    _check(lib.kg_cls_head_fwd(C.byref(a), _stream()), "kg_cls_head_fwd")
    return out


def cls_head_bwd(gtop: torch.Tensor, h: torch.Tensor, w1: torch.Tensor, w2: torch.Tensor, labels: torch.Tensor,
                 feat: torch.Tensor, logits: torch.Tensor, masked: bool = True, slope: float = 0.2):
    """The head's backward pass from the one-element device tensor ``gtop`` = d objective / d loss (kg_cls_head_bwd).  Returns
    (g, ws): the trunk's top gradient (N, C, T, V) - times lrelu'(h) when ``masked`` - and the workspace holding dlogits
    (N, L) and dfeat (N, F), the operand of cls_head_wgrad."""
    lib = load_library()
    _need_cuda(gtop, h, w1, w2, labels, feat, logits)
    f, l = w1.shape[0], w2.shape[0]
    a = _cls_head_args(*h.shape, f, l, slope)
    h = _bind(a, "h", "h", h, True)
    n, c = h.shape[0], h.shape[1]
    a.w1, a.w2 = _cls_flat(w1, f * c, torch.float32, "w1").data_ptr(), _cls_flat(w2, l * f, torch.float32, "w2").data_ptr()
    a.labels = _cls_flat(labels, n, torch.int64, "labels").data_ptr()
    a.feat, a.logits = _cls_flat(feat, n * f, torch.float32, "feat").data_ptr(), _cls_flat(logits, n * l, torch.float32, "logits").data_ptr()
    a.gtop, a.masked = _cls_flat(gtop, 1, torch.float32, "gtop").data_ptr(), int(bool(masked))
    g = _bind(a, "g", "g", new_plane(*h.shape, h.device))
    ws = _workspace("kg_cls_head_workspace_bytes", a, h.device)
    _check(lib.kg_cls_head_bwd(C.byref(a), _stream()), "kg_cls_head_bwd")
    return g, ws


def cls_head_wgrad(ws: torch.Tensor, pooled: torch.Tensor, feat: torch.Tensor, n_classes: int, dw1: torch.Tensor, db1: torch.Tensor,
                   dw2: torch.Tensor, db2: torch.Tensor, accumulate: bool = True) -> None:
    """dw1 (F, C), db1 (F), dw2 (L, F), db2 (L) (+)= the head's parameter gradients from the workspace cls_head_bwd filled
    and the forward's pooled (N, C) / feat (N, F) (kg_cls_head_wgrad)."""
    lib = load_library()
    _need_cuda(ws, pooled, feat, dw1, db1, dw2, db2)
    (n, c), f, l = pooled.shape, feat.shape[1], int(n_classes)
    a = _cls_head_args(n, c, 1, 1, f, l)
    a.pooled, a.feat = _cls_flat(pooled, n * c, torch.float32, "pooled").data_ptr(), _cls_flat(feat, n * f, torch.float32, "feat").data_ptr()
    a.dw1, a.db1 = _cls_flat(dw1, f * c, torch.float32, "dw1").data_ptr(), _cls_flat(db1, f, torch.float32, "db1").data_ptr()
    a.dw2, a.db2 = _cls_flat(dw2, l * f, torch.float32, "dw2").data_ptr(), _cls_flat(db2, l, torch.float32, "db2").data_ptr()
    a.accumulate = int(bool(accumulate))
    if ws.dtype != torch.float32 or not ws.is_contiguous():
        raise ValueError("kg_cls_head_wgrad: the workspace of cls_head_bwd expected")
    a.ws, a.ws_bytes = ws.data_ptr(), ws.numel() * 4
    _check(lib.kg_cls_head_wgrad(C.byref(a), _stream()), "kg_cls_head_wgrad")


def cls_scores(feats: Sequence[torch.Tensor], preds: Sequence[torch.Tensor], labels: torch.Tensor, div_pairs: torch.Tensor,
               mm_pairs: torch.Tensor, n_classes: int) -> dict:
    """Accuracy, per-class counts, diversity and multimodality of 1..CLS_MAX_SETS sets in ONE kg_cls_scores call (two
    launches, no host synchronisation, the same bits on every call).  ``feats``: (N, F) fp32 with unit column
    stride and one shared row stride (row slices of a wider matrix are read in place); ``preds``: (N,) int32; shared by the
    sets: ``labels`` (N,) int64, ``div_pairs`` (Sd, 2) and ``mm_pairs`` (n_classes * Sl, 2) int32 row indices
    (metrics.cls_pair_tables).  Returns device tensors: scores (S, 3) fp32 and scores64 (S, 3) fp64 = [accuracy, diversity,
    multimodality], correct (S,) int32, correct_per_class (S, K) int32, count_per_class (K,) int32, dist (S, Sd + K Sl) fp64."""
    lib = load_library()
    feats, preds, k = list(feats), list(preds), int(n_classes)
    s = len(feats)
    if len(preds) != s:
        raise ValueError(f"kg_cls_scores: {s} feature sets, {len(preds)} prediction vectors")
    if not 1 <= s <= CLS_MAX_SETS:       # (the library says so too; feats[0] below needs one set)
        raise ValueError(f"kg_cls_scores: nsets={s} outside [1, {CLS_MAX_SETS}]")
    _need_cuda(labels, div_pairs, mm_pairs, *feats, *preds)
    n, f = feats[0].shape
    ld = feats[0].stride(0) if n > 1 else max(f, feats[0].stride(0))
    for t in feats:
        if t.dtype != torch.float32 or tuple(t.shape) != (n, f) or (f > 1 and t.stride(1) != 1) or (n > 1 and t.stride(0) != ld):
            raise ValueError(f"kg_cls_scores: every feature set must be fp32 ({n}, {f}) with unit column stride and row stride {ld}")
    preds = [_cls_flat(t, n, torch.int32, "pred") for t in preds]
    labels = _cls_flat(labels, n, torch.int64, "labels")
    if div_pairs.dim() != 2 or div_pairs.shape[1] != 2 or mm_pairs.dim() != 2 or mm_pairs.shape[1] != 2 \
            or mm_pairs.shape[0] % max(k, 1):
        raise ValueError("kg_cls_scores: div_pairs (Sd, 2) and mm_pairs (n_classes * Sl, 2) expected")
    sd, sl = div_pairs.shape[0], mm_pairs.shape[0] // max(k, 1)
    div_pairs = _cls_flat(div_pairs, 2 * sd, torch.int32, "div_pairs")
    mm_pairs = _cls_flat(mm_pairs, 2 * k * sl, torch.int32, "mm_pairs")
    dev = feats[0].device
    out = dict(scores=torch.empty((s, 3), dtype=torch.float32, device=dev),
               scores64=torch.empty((s, 3), dtype=torch.float64, device=dev),
               correct=torch.empty(s, dtype=torch.int32, device=dev),
               correct_per_class=torch.empty((s, max(k, 1)), dtype=torch.int32, device=dev),
               count_per_class=torch.empty(max(k, 1), dtype=torch.int32, device=dev),
               dist=torch.empty((s, max(1, sd + k * sl)), dtype=torch.float64, device=dev))
    a = _ClsScoresArgs()
    a.nsets, a.N, a.F, a.K, a.Sd, a.Sl, a.feat_ld = s, n, f, k, sd, sl, ld
    for g in range(s):
        a.feat[g], a.pred[g] = feats[g].data_ptr(), preds[g].data_ptr()
    a.labels, a.div_pairs, a.mm_pairs = labels.data_ptr(), div_pairs.data_ptr(), mm_pairs.data_ptr()
    for key in ("dist", "scores64", "scores", "correct", "correct_per_class", "count_per_class"):
        setattr(a, key, out[key].data_ptr())
    _count("kg_cls_scores", 3.0 * s * (sd + k * sl) * f)
    _check(lib.kg_cls_scores(C.byref(a), _stream()), "kg_cls_scores")
    return out


def _label_bias_args(labels, emb, wg, K, C_out, cin, J, ak):
    a = _LabelBiasArgs()
    k, v, w = ak.shape
    assert k == K and ak.is_contiguous() and emb.is_contiguous() and labels.dtype == torch.int64 and labels.is_contiguous()
    a.N, a.L, a.J, a.K, a.C, a.V, a.W = labels.numel(), emb.shape[0], J, K, C_out, v, w
    a.labels, a.emb = labels.data_ptr(), emb.data_ptr()
    assert wg.is_contiguous()
    a.w, a.w_sK, a.w_sC = wg.data_ptr(), C_out * cin, cin
    a.ak = ak.data_ptr()
    return a


def label_bias_fwd(labels, emb, wg, K: int, C_out: int, cin: int, J: int, ak) -> torch.Tensor:
    """zl (N, C_out, 1, W): the bias the J label channels in front of block 0's input add to its gcn output
    (kg_label_bias_fwd).  wg: the gcn weight (K*C_out, cin, 1, 1) whose first J input columns multiply them."""
    lib = load_library()
    _need_cuda(labels, emb, wg, ak)
    a = _label_bias_args(labels, emb, wg, K, C_out, cin, J, ak)
    zl = torch.empty((labels.numel(), C_out, 1, ak.shape[2]), dtype=torch.float32, device=emb.device)
    a.zl = zl.data_ptr()
    ws = _workspace("kg_label_bias_workspace_bytes", a, emb.device)
    _check(lib.kg_label_bias_fwd(C.byref(a), _stream()), "kg_label_bias_fwd")
    return zl


def label_bias_bwd(gz, labels, emb, wg, K: int, C_out: int, cin: int, J: int, ak, demb=None, dw=None, dak=None,
                   accumulate: bool = True, dak_accumulate: bool = True):
    """First-order gradients of label_bias_fwd from gz (N, C_out, T, W) = d loss / d(gcn output): demb (L, J), dw (the gcn
    weight's gradient buffer, same addressing as wg) and dak (K, V, W) are written or (+)= (kg_label_bias_bwd)."""
    lib = load_library()
    gz = as_plane(gz)
    _need_cuda(gz, labels, emb, wg, ak, demb, dw, dak)
    a = _label_bias_args(labels, emb, wg, K, C_out, cin, J, ak)
    assert gz.shape[0] == labels.numel() and gz.shape[1] == C_out and gz.shape[3] == ak.shape[2]
    a.T = gz.shape[2]
    _bind(a, "gz", "gz", gz)
    for t in (demb, dw, dak):
        assert t is None or t.is_contiguous()
    a.demb, a.dw, a.dak = _ptr(demb), _ptr(dw), _ptr(dak)
    a.accumulate, a.dak_accumulate = int(bool(accumulate)), int(bool(dak_accumulate))
    ws = _workspace("kg_label_bias_workspace_bytes", a, gz.device)
    _check(lib.kg_label_bias_bwd(C.byref(a), _stream()), "kg_label_bias_bwd")


def mix3(real: torch.Tensor, fake: torch.Tensor, alpha: torch.Tensor) -> torch.Tensor:
    """(3n, C, T, V) = [real | fake | alpha real + (1 - alpha) fake], stored NCHW-contiguous (kg_mix3)"""
    lib = load_library()
    real, fake = as_plane(real), as_plane(fake)
    alpha = alpha.reshape(-1).contiguous()
    _need_cuda(real, fake, alpha)
    n, c, t, v = real.shape
    assert tuple(fake.shape) == (n, c, t, v) and alpha.numel() == n
    out = torch.empty((3 * n, c, t, v), dtype=torch.float32, device=real.device)
    a = _MixArgs()
    a.N, a.C, a.T, a.V = n, c, t, v
    _bind(a, "real", "r", real)
    _bind(a, "fake", "f", fake)
    a.alpha = alpha.data_ptr()
    a.out, a.o_sN, a.o_sC = out.data_ptr(), c * t * v, t * v          # (NCHW-contiguous, not channel-major)
    _check(lib.kg_mix3(C.byref(a), _stream()), "kg_mix3")
    return out


def masked_adj_fwd(A_all: torch.Tensor, imp_all: Optional[torch.Tensor], sel: Optional[torch.Tensor]) -> torch.Tensor:
    """ak = (A_all * imp_all)[sel] (flat; kg_masked_adj_fwd)"""
    lib = load_library()
    _need_cuda(A_all, imp_all, sel)
    n = sel.numel() if sel is not None else A_all.numel()
    ak = torch.empty(n, dtype=torch.float32, device=A_all.device)
    a = _MaskedAdjArgs()
    a.n = n
    a.a, a.imp, a.sel, a.ak = A_all.data_ptr(), _ptr(imp_all), _ptr(sel), ak.data_ptr()
    assert A_all.is_contiguous() and (imp_all is None or imp_all.is_contiguous()) and (sel is None or (sel.dtype == torch.int64 and sel.is_contiguous()))
    _check(lib.kg_masked_adj_fwd(C.byref(a), _stream()), "kg_masked_adj_fwd")
    return ak


def masked_adj_bwd(g: torch.Tensor, A_all: torch.Tensor, sel: Optional[torch.Tensor], dimp: torch.Tensor, accumulate: bool):
    """dimp[sel] (+)= g * A_all[sel] (kg_masked_adj_bwd); elements outside sel are not touched"""
    lib = load_library()
    g = g.reshape(-1).contiguous()
    _need_cuda(g, A_all, sel, dimp)
    a = _MaskedAdjArgs()
    a.n = g.numel()
    assert dimp.is_contiguous() and dimp.numel() == A_all.numel() and (sel is None or sel.numel() == g.numel())
    a.a, a.sel, a.g, a.dimp, a.accumulate = A_all.data_ptr(), _ptr(sel), g.data_ptr(), dimp.data_ptr(), int(bool(accumulate))
    _check(lib.kg_masked_adj_bwd(C.byref(a), _stream()), "kg_masked_adj_bwd")


# ---- label embedding + mapping network (kg_linear_fwd / kg_linear_bwd / kg_embed_bwd; generator.py:22-37,80-85) -------

def _linear_args(x, w, emb, labels):
    a = _LinearArgs()
    assert w.dim() == 2 and w.is_contiguous()
    a.Dout, a.Din = w.shape
    a.w = w.data_ptr()
    J = 0
    if emb is not None:
        assert emb.dim() == 2 and emb.is_contiguous() and labels is not None and labels.dtype == torch.int64 and labels.is_contiguous()
        a.L, J = emb.shape
        a.emb, a.labels = emb.data_ptr(), labels.data_ptr()
    a.J = J
    assert x.dim() == 2 and x.stride(1) == 1 and x.shape[1] == a.Din - J, (tuple(x.shape), a.Din, J)
    a.N = x.shape[0]
    a.x, a.x_ld = x.data_ptr(), x.stride(0)
    return a


def linear_fwd(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor], act: int = ACT_LRELU, slope: float = 0.2,
               emb: Optional[torch.Tensor] = None, labels: Optional[torch.Tensor] = None) -> torch.Tensor:
    """act(cat(emb[labels], x) @ w.T + b): one layer of the mapping network, the embedding lookup + cat of the first layer
    folded into its operand load (kg_linear_fwd)"""
    lib = load_library()
    _need_cuda(x, w, b, emb, labels)
    a = _linear_args(x, w, emb, labels)
    y = torch.empty(a.N, a.Dout, dtype=torch.float32, device=x.device)
    a.bias = _ptr(b)
    a.y, a.y_ld = y.data_ptr(), a.Dout
    a.act, a.slope = act, slope
    _check(lib.kg_linear_fwd(C.byref(a), _stream()), "kg_linear_fwd")
    return y


def linear_bwd(g: torch.Tensor, y: torch.Tensor, x: torch.Tensor, w: torch.Tensor, act: int = ACT_LRELU, slope: float = 0.2,
               emb: Optional[torch.Tensor] = None, labels: Optional[torch.Tensor] = None, gx_cols: Optional[int] = None,
               dw: Optional[torch.Tensor] = None, db: Optional[torch.Tensor] = None, accumulate: bool = False):
    """One layer's backward pass in ONE launch (kg_linear_bwd): returns gx (N, gx_cols) (None for 0 columns; default: all
    Din); writes / adds dw (Dout, Din) and db (Dout) when given."""
    lib = load_library()
    _need_cuda(g, y, x, w, emb, labels, dw, db)
    a = _linear_args(x, w, emb, labels)
    assert g.shape == (a.N, a.Dout) and y.shape == (a.N, a.Dout) and g.stride(1) == 1 and y.stride(1) == 1
    a.g, a.g_ld = g.data_ptr(), g.stride(0)
    a.y, a.y_ld = y.data_ptr(), y.stride(0)
    a.act, a.slope = act, slope
    cols = a.Din if gx_cols is None else gx_cols
    gx = None
    if cols > 0:
        gx = torch.empty(a.N, cols, dtype=torch.float32, device=g.device)
        a.gx, a.gx_ld = gx.data_ptr(), cols
    a.gx_cols = cols
    if dw is not None:
        assert dw.is_contiguous() and dw.numel() == a.Dout * a.Din
    if db is not None:
        assert db.is_contiguous() and db.numel() == a.Dout
    a.dw, a.db, a.accumulate = _ptr(dw), _ptr(db), int(bool(accumulate))
    _check(lib.kg_linear_bwd(C.byref(a), _stream()), "kg_linear_bwd")
    return gx


def embed_bwd(gx: torch.Tensor, labels: torch.Tensor, demb: torch.Tensor, accumulate: bool = False):
    """demb[l] (+)= sum of gx[n] over the samples of class l, in index order (kg_embed_bwd)"""
    lib = load_library()
    _need_cuda(gx, labels, demb)
    a = _LinearArgs()
    assert gx.dim() == 2 and gx.stride(1) == 1 and demb.dim() == 2 and demb.is_contiguous() and demb.shape[1] <= gx.shape[1]
    assert labels.dtype == torch.int64 and labels.is_contiguous()
    a.N = gx.shape[0]
    a.L, a.J = demb.shape
    a.gx, a.gx_ld = gx.data_ptr(), gx.stride(0)
    a.labels, a.demb, a.accumulate = labels.data_ptr(), demb.data_ptr(), int(bool(accumulate))
    _check(lib.kg_embed_bwd(C.byref(a), _stream()), "kg_embed_bwd")


# ---- data-parallel gradient exchange (kg_comm_*: RCCL over xGMI behind the C ABI) -------------------------------------

COMM_ID_BYTES = 128


# ---- MMD evaluation ----------------------------------------------------------------------------------------------------

class MmdView(NamedTuple):
    """How kg_mmd walks one operand: element (class c, group f, point i, dimension d) sits at
    t.data_ptr() + (c*sc + f*sg + i*sp + d*sd) floats."""
    t: torch.Tensor
    sp: int
    sd: int
    sg: int
    sc: int


def _mmd_extent_ok(v: MmdView, m: int, dim: int, groups: int, classes: int) -> bool:
    """every element kg_mmd will read lies inside the tensor's storage"""
    if min(v.sp, v.sd, v.sg, v.sc) < 0:
        return False
    last = (classes - 1) * v.sc + (groups - 1) * v.sg + (m - 1) * v.sp + (dim - 1) * v.sd
    return v.t.storage_offset() + last < v.t.untyped_storage().nbytes() // 4


def mmd(x: MmdView, y: MmdView, m: int, n: int, dim: int, groups: int, classes: int,
        bandwidths: Sequence[float], want_mean: bool = False) -> dict:
    """Enqueue kg_mmd (pair sums of every (group, bandwidth) + the finishing launch) on the current stream; no host
    synchronisation.  Returns dict(mmd2 (classes*groups, nbw), mmd (classes, nbw), result (classes,), mean (0-d or
    None)), all fp32 on the device."""
    lib = load_library()
    for v in (x, y):
        if v.t.dtype != torch.float32:
            raise TypeError(f"kg_mmd: fp32 only, got {v.t.dtype}")
    _need_cuda(x.t, y.t)
    bws = [float(b) for b in bandwidths]
    a = _MmdArgs()
    a.x, a.x_sp, a.x_sd, a.x_sg, a.x_sc = x.t.data_ptr(), x.sp, x.sd, x.sg, x.sc
    a.y, a.y_sp, a.y_sd, a.y_sg, a.y_sc = y.t.data_ptr(), y.sp, y.sd, y.sg, y.sc
    a.m, a.n, a.dim, a.groups, a.classes, a.nbw = int(m), int(n), int(dim), int(groups), int(classes), len(bws)
    for i, b in enumerate(bws[:MMD_MAX_BW]):
        a.bw[i] = b
    nbytes = _query("kg_mmd_workspace_bytes", a)
    for name, v, p in (("x", x, m), ("y", y, n)):
        if not _mmd_extent_ok(v, p, dim, groups, classes):
            raise ValueError(f"kg_mmd: the strides of {name} reach outside its tensor")
    dev = x.t.device
    ws = torch.empty(max(1, nbytes // 4), dtype=torch.float32, device=dev)
    out = dict(mmd2=torch.empty((classes * groups, len(bws)), dtype=torch.float32, device=dev),
               mmd=torch.empty((classes, len(bws)), dtype=torch.float32, device=dev),
               result=torch.empty(classes, dtype=torch.float32, device=dev),
               mean=torch.empty((), dtype=torch.float32, device=dev) if want_mean else None)
    a.mmd2, a.mmd, a.result = out["mmd2"].data_ptr(), out["mmd"].data_ptr(), out["result"].data_ptr()
    a.mean = _ptr(out["mean"])
    a.ws, a.ws_bytes = ws.data_ptr(), ws.numel() * 4
    _count("kg_mmd", 3.0 * 2.0 * m * (m - 1) * dim * groups * classes)
    _check(lib.kg_mmd(C.byref(a), _stream()), "kg_mmd")
    return out


# ---- precision / recall / density / coverage (kg_prdc.hip) ----------------------------------------------------------------

class PrdcView(NamedTuple):
    """How kg_prdc walks one set: element (class c, point i, outer o, inner e) sits at
    t.data_ptr() + (c*sc + i*sp + o*so + e) floats."""
    t: torch.Tensor
    sc: int
    sp: int
    so: int


def _prdc_extent_ok(v: PrdcView, pts: int, d_outer: int, d_inner: int, classes: int) -> bool:
    """every element kg_prdc will read lies inside the tensor's storage"""
    if min(v.sc, v.sp, v.so) < 0:
        return False
    last = (classes - 1) * v.sc + (pts - 1) * v.sp + (d_outer - 1) * v.so + d_inner - 1
    return v.t.storage_offset() + last < v.t.untyped_storage().nbytes() // 4


def prdc_workspace_bytes(n: int, m: int, d_outer: int, d_inner: int, classes: int, k: int) -> int:
    """kg_prdc_workspace_bytes of a shape (RuntimeError naming the field for a shape kg_prdc rejects); no GPU call"""
    a = _PrdcArgs()
    a.n, a.m, a.d_outer, a.d_inner, a.classes, a.k = int(n), int(m), int(d_outer), int(d_inner), int(classes), int(k)
    return _query("kg_prdc_workspace_bytes", a)


def prdc(real: PrdcView, fake: PrdcView, n: int, m: int, d_outer: int, d_inner: int, classes: int, k: int,
         want_mean: bool = True, per_point: bool = False, ws: Optional[torch.Tensor] = None) -> dict:
    """Enqueue kg_prdc (radii, cross and finishing launch) on the current stream; no host synchronisation.  Returns
    dict(counts (classes, 4) int32, values (classes, 4) fp32, mean (4,) fp32 or None) on the device; with ``per_point``
    also radii_real (classes, n), radii_fake (classes, m), fake_hits (classes, m) int32 and real_flags (classes, n)
    uint8.  ``ws``: a caller's workspace (any dtype of 4-byte elements, at least the needed bytes; its contents do not
    matter), else one is taken with torch.empty."""
    lib = load_library()
    for v in (real, fake):
        if v.t.dtype != torch.float32:
            raise TypeError(f"kg_prdc: fp32 only, got {v.t.dtype}")
    nbytes = prdc_workspace_bytes(n, m, d_outer, d_inner, classes, k)
    _need_cuda(real.t, fake.t, ws)
    for name, v, p in (("real", real, n), ("fake", fake, m)):
        if not _prdc_extent_ok(v, p, d_outer, d_inner, classes):
            raise ValueError(f"kg_prdc: the strides of {name} reach outside its tensor")
    dev = real.t.device
    if ws is None:
        ws = torch.empty(max(1, nbytes // 4), dtype=torch.int32, device=dev)
    elif not ws.is_contiguous() or ws.element_size() != 4:
        raise ValueError("kg_prdc: ws must be a contiguous tensor of 4-byte elements")
    out = dict(counts=torch.empty((classes, 4), dtype=torch.int32, device=dev),
               values=torch.empty((classes, 4), dtype=torch.float32, device=dev),
               mean=torch.empty(4, dtype=torch.float32, device=dev) if want_mean else None)
    if per_point:
        out.update(radii_real=torch.empty((classes, n), dtype=torch.float32, device=dev),
                   radii_fake=torch.empty((classes, m), dtype=torch.float32, device=dev),
                   fake_hits=torch.empty((classes, m), dtype=torch.int32, device=dev),
                   real_flags=torch.empty((classes, n), dtype=torch.uint8, device=dev))
    a = _PrdcArgs()
    a.real, a.r_sc, a.r_sp, a.r_so = real.t.data_ptr(), real.sc, real.sp, real.so
    a.fake, a.f_sc, a.f_sp, a.f_so = fake.t.data_ptr(), fake.sc, fake.sp, fake.so
    a.n, a.m, a.d_outer, a.d_inner, a.classes, a.k = int(n), int(m), int(d_outer), int(d_inner), int(classes), int(k)
    a.radii_real, a.radii_fake = _ptr(out.get("radii_real")), _ptr(out.get("radii_fake"))
    a.fake_hits, a.real_flags = _ptr(out.get("fake_hits")), _ptr(out.get("real_flags"))
    a.counts, a.values, a.mean = out["counts"].data_ptr(), out["values"].data_ptr(), _ptr(out["mean"])
    a.ws, a.ws_bytes = ws.data_ptr(), ws.numel() * 4
    _count("kg_prdc", 3.0 * (float(n) * n + float(m) * m + float(n) * m) * d_outer * d_inner * classes)
    _check(lib.kg_prdc(C.byref(a), _stream()), "kg_prdc")
    return out


def prdc_radii(x: PrdcView, n: int, d_outer: int, d_inner: int, classes: int, k: int,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Enqueue kg_prdc_radii: the (classes, n) squared k-th-neighbour radii of ONE point set (one launch, no workspace);
    ``out``: a contiguous fp32 tensor of classes * n elements to write into, else one is taken with torch.empty."""
    if x.t.dtype != torch.float32:
        raise TypeError(f"kg_prdc_radii: fp32 only, got {x.t.dtype}")
    _need_cuda(x.t, out)
    if min(n, d_outer, d_inner, classes) >= 1 and not _prdc_extent_ok(x, n, d_outer, d_inner, classes):
        raise ValueError("kg_prdc_radii: the strides of x reach outside its tensor")
    if out is None:
        out = torch.empty((max(classes, 0), max(n, 0)), dtype=torch.float32, device=x.t.device)
    else:
        _dest(out, classes * n, "kg_prdc_radii: out must be a contiguous fp32 tensor of classes * n elements")
    a = _PrdcRadiiArgs()
    a.x, a.sc, a.sp, a.so = x.t.data_ptr(), x.sc, x.sp, x.so
    a.n, a.d_outer, a.d_inner, a.classes, a.k = int(n), int(d_outer), int(d_inner), int(classes), int(k)
    a.radii = out.data_ptr()
    _count("kg_prdc_radii", 3.0 * float(n) * n * d_outer * d_inner * classes)
    _check(load_library().kg_prdc_radii(C.byref(a), _stream()), "kg_prdc_radii")
    return out


def prdc_sets_workspace_bytes(nsets: int, n: int, m: int, d_outer: int, d_inner: int, classes: int, k: int) -> int:
    """kg_prdc_sets_workspace_bytes of a shape = 4 nsets classes (2 m + n) (RuntimeError naming the field for a shape
    kg_prdc_sets rejects); no GPU call"""
    a = _PrdcSetsArgs()
    a.nsets, a.n, a.m = int(nsets), int(n), int(m)
    a.d_outer, a.d_inner, a.classes, a.k = int(d_outer), int(d_inner), int(classes), int(k)
    return _query("kg_prdc_sets_workspace_bytes", a)


def prdc_sets(real: PrdcView, fakes: Sequence[torch.Tensor], f_sc: int, f_sp: int, f_so: int, radii_real: torch.Tensor,
              n: int, m: int, d_outer: int, d_inner: int, classes: int, k: int, want_mean: bool = True,
              per_point: bool = False, ws: Optional[torch.Tensor] = None) -> dict:
    """Enqueue kg_prdc_sets: the ``fakes`` (1..PRDC_MAX_SETS fp32 tensors walked with the shared strides f_sc / f_sp /
    f_so) against ONE real set whose (classes, n) radii ``radii_real`` are an input (``prdc_radii``); three launches
    whatever the number of sets, no host synchronisation.  Returns dict(counts (nsets, classes, 4) int32, values (nsets,
    classes, 4) fp32, mean (nsets, 4) fp32 or None) on the device; with ``per_point`` also radii_fake (nsets, classes, m),
    fake_hits (nsets, classes, m) int32 and real_flags (nsets, classes, n) uint8.  Every entry of set g equals, bit for
    bit, that of ``prdc(real, fakes[g])``.  ``ws`` as in ``prdc``."""
    lib = load_library()
    fakes = list(fakes)
    for t in [real.t, radii_real] + fakes:
        if t.dtype != torch.float32:
            raise TypeError(f"kg_prdc_sets: fp32 only, got {t.dtype}")
    nsets = len(fakes)
    nbytes = prdc_sets_workspace_bytes(nsets, n, m, d_outer, d_inner, classes, k)
    _need_cuda(real.t, radii_real, ws, *fakes)
    if not _prdc_extent_ok(real, n, d_outer, d_inner, classes):
        raise ValueError("kg_prdc_sets: the strides of real reach outside its tensor")
    for g, t in enumerate(fakes):
        if not _prdc_extent_ok(PrdcView(t, f_sc, f_sp, f_so), m, d_outer, d_inner, classes):
            raise ValueError(f"kg_prdc_sets: the strides of fake set {g} reach outside its tensor")
    if not radii_real.is_contiguous() or radii_real.numel() != classes * n:
        raise ValueError("kg_prdc_sets: radii_real must be a contiguous fp32 tensor of classes * n elements")
    dev = real.t.device
    if ws is None:
        ws = torch.empty(max(1, nbytes // 4), dtype=torch.int32, device=dev)
    elif not ws.is_contiguous() or ws.element_size() != 4:
        raise ValueError("kg_prdc_sets: ws must be a contiguous tensor of 4-byte elements")
    out = dict(counts=torch.empty((nsets, classes, 4), dtype=torch.int32, device=dev),
               values=torch.empty((nsets, classes, 4), dtype=torch.float32, device=dev),
               mean=torch.empty((nsets, 4), dtype=torch.float32, device=dev) if want_mean else None)
    if per_point:
        out.update(radii_fake=torch.empty((nsets, classes, m), dtype=torch.float32, device=dev),
                   fake_hits=torch.empty((nsets, classes, m), dtype=torch.int32, device=dev),
                   real_flags=torch.empty((nsets, classes, n), dtype=torch.uint8, device=dev))
    a = _PrdcSetsArgs()
    a.real, a.r_sc, a.r_sp, a.r_so = real.t.data_ptr(), real.sc, real.sp, real.so
    for g, t in enumerate(fakes):
        a.fake[g] = t.data_ptr()
    a.f_sc, a.f_sp, a.f_so = int(f_sc), int(f_sp), int(f_so)
    a.nsets, a.n, a.m = nsets, int(n), int(m)
    a.d_outer, a.d_inner, a.classes, a.k = int(d_outer), int(d_inner), int(classes), int(k)
    a.radii_real, a.radii_fake = radii_real.data_ptr(), _ptr(out.get("radii_fake"))
    a.fake_hits, a.real_flags = _ptr(out.get("fake_hits")), _ptr(out.get("real_flags"))
    a.counts, a.values, a.mean = out["counts"].data_ptr(), out["values"].data_ptr(), _ptr(out["mean"])
    a.ws, a.ws_bytes = ws.data_ptr(), ws.numel() * 4
    _count("kg_prdc_sets", 3.0 * nsets * (float(m) * m + float(n) * m) * d_outer * d_inner * classes)
    _check(lib.kg_prdc_sets(C.byref(a), _stream()), "kg_prdc_sets")
    return out


# ---- exact k nearest neighbours between two point sets (kg_nn.hip) --------------------------------------------------------

def _nn_shape(a: "_NnArgs", Q, N, d_outer, d_inner, classes, k, exclude_self, q_affine, b_affine, tile, split):
    a.Q, a.N, a.d_outer, a.d_inner, a.classes, a.k = int(Q), int(N), int(d_outer), int(d_inner), int(classes), int(k)
    a.tile, a.split = int(tile), int(split)
    if exclude_self is not None:                # (None: a struct without the field - the sets)
        a.exclude_self = int(bool(exclude_self))
    for pre, aff in (("q", q_affine), ("b", b_affine)):
        if aff is not None:
            setattr(a, pre + "_affine", 1)
            setattr(a, pre + "_scale", float(aff[0]))
            setattr(a, pre + "_shift", float(aff[1]))


def nn_workspace_bytes(Q: int, N: int, d_outer: int, d_inner: int, classes: int, k: int, exclude_self: bool = False,
                       tile: int = 0, split: int = 0) -> int:
    """kg_nn_workspace_bytes of a shape = classes * Q * split * k * 8 with the plan's split (RuntimeError naming the field for
    a shape kg_nn rejects); no GPU call"""
    a = _NnArgs()
    _nn_shape(a, Q, N, d_outer, d_inner, classes, k, exclude_self, None, None, tile, split)
    return _query("kg_nn_workspace_bytes", a)


def nn(query: PrdcView, base: PrdcView, Q: int, N: int, d_outer: int, d_inner: int, classes: int, k: int,
       exclude_self: bool = False, q_affine: Optional[Tuple[float, float]] = None,
       b_affine: Optional[Tuple[float, float]] = None, tile: int = 0, split: int = 0,
       ws: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Enqueue kg_nn (search and merge launch) on the current stream; no host synchronisation.  For every class and query
    the k base points with the smallest (squared distance, index): returns (idx (classes, Q, k) int32 - the base index
    inside the class -, d2 (classes, Q, k) fp32) on the device.  ``query`` / ``base``: how each side is walked (the views of
    ``prdc``); ``exclude_self``: pair i == j is left out by index; ``q_affine`` / ``b_affine``: (scale, shift), that side
    is read as (x * scale) + shift in two roundings; ``tile`` / ``split``: 0 or a forced plan (same bits under every plan);
    ``ws`` as in ``prdc``."""
    for v in (query, base):
        if v.t.dtype != torch.float32:
            raise TypeError(f"kg_nn: fp32 only, got {v.t.dtype}")
    a = _NnArgs()
    _nn_shape(a, Q, N, d_outer, d_inner, classes, k, exclude_self, q_affine, b_affine, tile, split)
    nbytes = _query("kg_nn_workspace_bytes", a)
    _need_cuda(query.t, base.t, ws)
    for name, v, p in (("query", query, Q), ("base", base, N)):
        if not _prdc_extent_ok(v, p, d_outer, d_inner, classes):
            raise ValueError(f"kg_nn: the strides of {name} reach outside its tensor")
    dev = query.t.device
    if ws is None:
        ws = _workspace("kg_nn_workspace_bytes", a, dev)
    elif not ws.is_contiguous() or ws.element_size() != 4 or ws.numel() * 4 < nbytes:
        raise ValueError("kg_nn: ws must be a contiguous tensor of 4-byte elements, at least %d bytes" % nbytes)
    else:
        a.ws, a.ws_bytes = ws.data_ptr(), ws.numel() * 4
    idx = torch.empty((classes, Q, k), dtype=torch.int32, device=dev)
    d2 = torch.empty((classes, Q, k), dtype=torch.float32, device=dev)
    a.query, a.q_sc, a.q_sp, a.q_so = query.t.data_ptr(), query.sc, query.sp, query.so
    a.base, a.b_sc, a.b_sp, a.b_so = base.t.data_ptr(), base.sc, base.sp, base.so
    a.idx, a.d2 = idx.data_ptr(), d2.data_ptr()
    _count("kg_nn", 3.0 * float(Q) * N * d_outer * d_inner * classes)
    _check(load_library().kg_nn(C.byref(a), _stream()), "kg_nn")
    return idx, d2


def nn_sets_workspace_bytes(nsets: int, Q: int, N: int, d_outer: int, d_inner: int, classes: int, k: int, tile: int = 0,
                            split: int = 0) -> int:
    """kg_nn_sets_workspace_bytes of a shape = nsets * classes * Q * split * k * 8 with the plan's split (RuntimeError naming
    the field for a shape kg_nn_sets rejects); no GPU call"""
    a = _NnSetsArgs()
    a.nsets = int(nsets)
    _nn_shape(a, Q, N, d_outer, d_inner, classes, k, None, None, None, tile, split)
    return _query("kg_nn_sets_workspace_bytes", a)


def nn_sets(queries: Sequence[torch.Tensor], q_sc: int, q_sp: int, q_so: int, base: PrdcView, Q: int, N: int, d_outer: int,
            d_inner: int, classes: int, k: int, q_affine: Optional[Tuple[float, float]] = None,
            b_affine: Optional[Tuple[float, float]] = None, tile: int = 0, split: int = 0,
            ws: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Enqueue kg_nn_sets: the ``queries`` (1..NN_MAX_SETS fp32 tensors walked with the shared strides q_sc / q_sp / q_so and
    the shared ``q_affine``) against ONE base in two launches whatever the number of sets; no host synchronisation.  Returns
    (idx (nsets, classes, Q, k) int32, d2 (nsets, classes, Q, k) fp32) on the device; set g equals, bit for bit,
    ``nn(PrdcView(queries[g], ...), base)``.  The other arguments as in ``nn`` (there is no ``exclude_self``)."""
    queries = list(queries)
    for t in queries + [base.t]:
        if t.dtype != torch.float32:
            raise TypeError(f"kg_nn_sets: fp32 only, got {t.dtype}")
    nsets = len(queries)
    a = _NnSetsArgs()
    a.nsets = nsets
    _nn_shape(a, Q, N, d_outer, d_inner, classes, k, None, q_affine, b_affine, tile, split)
    nbytes = _query("kg_nn_sets_workspace_bytes", a)
    _need_cuda(base.t, ws, *queries)
    for g, t in enumerate(queries):
        if not _prdc_extent_ok(PrdcView(t, q_sc, q_sp, q_so), Q, d_outer, d_inner, classes):
            raise ValueError(f"kg_nn_sets: the strides of query set {g} reach outside its tensor")
    if not _prdc_extent_ok(base, N, d_outer, d_inner, classes):
        raise ValueError("kg_nn_sets: the strides of base reach outside its tensor")
    dev = base.t.device
    if ws is None:
        ws = _workspace("kg_nn_sets_workspace_bytes", a, dev)
    elif not ws.is_contiguous() or ws.element_size() != 4 or ws.numel() * 4 < nbytes:
        raise ValueError("kg_nn_sets: ws must be a contiguous tensor of 4-byte elements, at least %d bytes" % nbytes)
    else:
        a.ws, a.ws_bytes = ws.data_ptr(), ws.numel() * 4
    idx = torch.empty((nsets, classes, Q, k), dtype=torch.int32, device=dev)
    d2 = torch.empty((nsets, classes, Q, k), dtype=torch.float32, device=dev)
    for g, t in enumerate(queries):
        a.query[g] = t.data_ptr()
    a.q_sc, a.q_sp, a.q_so = int(q_sc), int(q_sp), int(q_so)
    a.base, a.b_sc, a.b_sp, a.b_so = base.t.data_ptr(), base.sc, base.sp, base.so
    a.idx, a.d2 = idx.data_ptr(), d2.data_ptr()
    _count("kg_nn_sets", 3.0 * nsets * float(Q) * N * d_outer * d_inner * classes)
    _check(load_library().kg_nn_sets(C.byref(a), _stream()), "kg_nn_sets")
    return idx, d2


def nn_scores(idx: torch.Tensor, d2: torch.Tensor, query_labels: torch.Tensor, base_labels: torch.Tensor,
              base_loo: torch.Tensor, n_classes: int, per_class: bool = False) -> dict:
    """Enqueue kg_nn_scores (ONE launch): the memorisation tallies of 1..NN_MAX_SETS sets from their nearest neighbours.
    ``idx`` int32 / ``d2`` fp32: (nsets, Q), or (nsets, Q, k) / (nsets, 1, Q, k) results of ``nn_sets`` whose column 0 is
    read in place; ``query_labels`` (Q,) int32 shared by the sets, ``base_labels`` (N,) int32, ``base_loo`` (N,) fp32 - the
    leave-one-out nearest squared distance of every base point.  Returns device tensors counts (nsets, 2) int64 (authentic,
    agreeing), scores64 (nsets, 2), scores (nsets, 2) fp32 = the one rounding of counts / Q, and with ``per_class``
    counts_per_class (nsets, n_classes, 2) int32 by the query's label.  No host synchronisation."""
    who = "kg_nn_scores"
    if idx.dim() == 4 and idx.shape[1] == 1:
        idx, d2 = idx[:, 0], d2[:, 0]
    if idx.dim() == 3:
        idx, d2 = idx[:, :, 0], d2[:, :, 0]
    if idx.dim() != 2 or idx.shape != d2.shape or idx.dtype != torch.int32 or d2.dtype != torch.float32:
        raise ValueError(f"{who}: idx int32 and d2 fp32 of one shape (nsets, Q[, k]) expected")
    nsets, Q = idx.shape
    ld = idx.stride(1) if Q > 1 else 1
    for t in (idx, d2):
        if (Q > 1 and t.stride(1) != ld) or (nsets > 1 and t.stride(0) != Q * ld) or ld < 1:
            raise ValueError(f"{who}: idx / d2 must be (nsets, Q) views with strides (Q * ld, ld)")
    for name, t, dt in (("query_labels", query_labels, torch.int32), ("base_labels", base_labels, torch.int32),
                        ("base_loo", base_loo, torch.float32)):
        if t.dim() != 1 or t.dtype != dt or not t.is_contiguous():
            raise ValueError(f"{who}: {name} must be a contiguous 1-D {dt} tensor")
    if query_labels.shape[0] != Q or base_labels.shape[0] != base_loo.shape[0]:
        raise ValueError(f"{who}: {query_labels.shape[0]} query_labels for Q={Q}, {base_labels.shape[0]} base_labels for "
                         f"{base_loo.shape[0]} base_loo")
    _need_cuda(idx, d2, query_labels, base_labels, base_loo)
    dev = idx.device
    out = dict(counts=torch.empty((nsets, 2), dtype=torch.int64, device=dev),
               scores64=torch.empty((nsets, 2), dtype=torch.float64, device=dev),
               scores=torch.empty((nsets, 2), dtype=torch.float32, device=dev))
    if per_class:
        out["counts_per_class"] = torch.empty((nsets, max(int(n_classes), 0), 2), dtype=torch.int32, device=dev)
    a = _NnScoresArgs()
    a.nsets, a.Q, a.N, a.n_classes, a.ld = nsets, Q, base_loo.shape[0], int(n_classes), ld
    a.idx, a.d2 = idx.data_ptr(), d2.data_ptr()
    a.query_labels, a.base_labels, a.base_loo = query_labels.data_ptr(), base_labels.data_ptr(), base_loo.data_ptr()
    a.counts, a.counts_per_class = out["counts"].data_ptr(), _ptr(out.get("counts_per_class"))
    a.scores64, a.scores = out["scores64"].data_ptr(), out["scores"].data_ptr()
    _count(who, 0.0)
    _check(load_library().kg_nn_scores(C.byref(a), _stream()), who)
    return out


# ---- matrix-core pre-filter with exact re-score (kg_nn_gram.hip) ---------------------------------------------

def nn_norms(x: PrdcView, n: int, d_outer: int, d_inner: int, classes: int,
             affine: Optional[Tuple[float, float]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Enqueue kg_nn_norms (ONE launch): (norms (classes, n), parts (classes, NN_NORM_PARTS)) fp32 - the squared norm of every
    point of the set as ``nn_gram`` reads it (strides, ``affine``) and the largest of them in NN_NORM_PARTS parts per class
    (``parts.amax(1)`` is the class's largest norm).  Computed once for a base that does not change."""
    if x.t.dtype != torch.float32:
        raise TypeError(f"kg_nn_norms: fp32 only, got {x.t.dtype}")
    _need_cuda(x.t)
    if min(n, d_outer, d_inner, classes) >= 1 and not _prdc_extent_ok(x, n, d_outer, d_inner, classes):
        raise ValueError("kg_nn_norms: the strides of x reach outside its tensor")
    a = _NnGramArgs()
    a.base, a.b_sc, a.b_sp, a.b_so = x.t.data_ptr(), x.sc, x.sp, x.so
    a.N, a.d_outer, a.d_inner, a.classes = int(n), int(d_outer), int(d_inner), int(classes)
    if affine is not None:
        a.b_affine, a.b_scale, a.b_shift = 1, float(affine[0]), float(affine[1])
    norms = torch.empty((max(classes, 0), max(n, 0)), dtype=torch.float32, device=x.t.device)
    parts = torch.empty((max(classes, 0), NN_NORM_PARTS), dtype=torch.float32, device=x.t.device)
    _count("kg_nn_norms", 2.0 * float(n) * d_outer * d_inner * classes)
    _check(load_library().kg_nn_norms(C.byref(a), norms.data_ptr(), parts.data_ptr(), _stream()), "kg_nn_norms")
    return norms, parts


def nn_gram_workspace_bytes(nsets: int, Q: int, N: int, d_outer: int, d_inner: int, classes: int, k: int,
                            exclude_self: bool = False, cand: int = 0, tile: int = 0, split: int = 0) -> int:
    """kg_nn_gram_workspace_bytes of a shape = nsets * classes * (Q * (8 * cand * (split + 1) + 8) + 4) with the plan's split
    and cand (RuntimeError naming the field for a shape kg_nn_gram rejects); no GPU call"""
    a = _NnGramArgs()
    a.nsets, a.cand = int(nsets), int(cand)
    _nn_shape(a, Q, N, d_outer, d_inner, classes, k, exclude_self, None, None, tile, split)
    return _query("kg_nn_gram_workspace_bytes", a)


def nn_gram(queries: Sequence[torch.Tensor], q_sc: int, q_sp: int, q_so: int, base: PrdcView, Q: int, N: int, d_outer: int,
            d_inner: int, classes: int, k: int, exclude_self: bool = False, q_affine: Optional[Tuple[float, float]] = None,
            b_affine: Optional[Tuple[float, float]] = None, cand: int = 0, tile: int = 0, split: int = 0,
            base_norms: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
            ws: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Enqueue kg_nn_gram: the results of ``nn_sets`` (of ``nn`` with ``exclude_self``, one set), bit for bit, through the
    matrix-core pre-filter with exact re-score and fallback - six launches, no host synchronisation.  Returns (idx (nsets,
    classes, Q, k) int32, d2 (nsets, classes, Q, k) fp32, stats (nsets, classes, 2) int32: certified rows, fallback rows) on
    the device.  ``base_norms``: ``nn_norms`` of the base (same view and affine) - without it that launch is made here;
    ``cand``: 0 or a forced number of candidates per row (k < cand <= NN_MAX_K).  The other arguments as in ``nn_sets``."""
    queries = list(queries)
    for t in queries + [base.t]:
        if t.dtype != torch.float32:
            raise TypeError(f"kg_nn_gram: fp32 only, got {t.dtype}")
    nsets = len(queries)
    a = _NnGramArgs()
    a.nsets, a.cand = nsets, int(cand)
    _nn_shape(a, Q, N, d_outer, d_inner, classes, k, exclude_self, q_affine, b_affine, tile, split)
    nbytes = _query("kg_nn_gram_workspace_bytes", a)
    _need_cuda(base.t, ws, *queries)
    for g, t in enumerate(queries):
        if not _prdc_extent_ok(PrdcView(t, q_sc, q_sp, q_so), Q, d_outer, d_inner, classes):
            raise ValueError(f"kg_nn_gram: the strides of query set {g} reach outside its tensor")
    if not _prdc_extent_ok(base, N, d_outer, d_inner, classes):
        raise ValueError("kg_nn_gram: the strides of base reach outside its tensor")
    dev = base.t.device
    if base_norms is None:
        base_norms = nn_norms(base, N, d_outer, d_inner, classes, b_affine)
    norms, parts = base_norms
    for t, n, name in ((norms, classes * N, "norms (classes, N)"), (parts, classes * NN_NORM_PARTS, "parts (classes, %d)" % NN_NORM_PARTS)):
        _need_cuda(t)
        _dest(t, n, "kg_nn_gram: base_norms[...] %s must be a contiguous fp32 tensor" % name)
    if ws is None:
        ws = _workspace("kg_nn_gram_workspace_bytes", a, dev)
    elif not ws.is_contiguous() or ws.element_size() != 4 or ws.numel() * 4 < nbytes:
        raise ValueError("kg_nn_gram: ws must be a contiguous tensor of 4-byte elements, at least %d bytes" % nbytes)
    else:
        a.ws, a.ws_bytes = ws.data_ptr(), ws.numel() * 4
    idx = torch.empty((nsets, classes, Q, k), dtype=torch.int32, device=dev)
    d2 = torch.empty((nsets, classes, Q, k), dtype=torch.float32, device=dev)
    stats = torch.empty((nsets, classes, 2), dtype=torch.int32, device=dev)
    for g, t in enumerate(queries):
        a.query[g] = t.data_ptr()
    a.q_sc, a.q_sp, a.q_so = int(q_sc), int(q_sp), int(q_so)
    a.base, a.b_sc, a.b_sp, a.b_so = base.t.data_ptr(), base.sc, base.sp, base.so
    a.b_norms, a.b_norm_parts = norms.data_ptr(), parts.data_ptr()
    a.idx, a.d2, a.stats = idx.data_ptr(), d2.data_ptr(), stats.data_ptr()
    _count("kg_nn_gram", 2.0 * nsets * float(Q) * N * d_outer * d_inner * classes)
    _check(load_library().kg_nn_gram(C.byref(a), _stream()), "kg_nn_gram")
    return idx, d2, stats


# ---- Frechet distance of pose / motion / caller features (kg_frechet.hip) -------------------------------------------------

class FrechetView(NamedTuple):
    """How kg_frechet walks one set: element (class c, sample i, frame f, outer o, inner e) sits at
    t.data_ptr() + (c*sc + i*ss + f*sf + o*so + e) floats."""
    t: torch.Tensor
    sc: int
    ss: int
    sf: int
    so: int


def _frechet_extent_ok(v: FrechetView, samples: int, frames: int, d_outer: int, d_inner: int, classes: int) -> bool:
    """every element kg_frechet will read lies inside the tensor's storage"""
    if min(v.sc, v.ss, v.sf, v.so) < 0:
        return False
    last = (classes - 1) * v.sc + (samples - 1) * v.ss + (frames - 1) * v.sf + (d_outer - 1) * v.so + d_inner - 1
    return v.t.storage_offset() + last < v.t.untyped_storage().nbytes() // 4


def _frechet_shape(n: int, m: int, frames: int, diff: bool, d_outer: int, d_inner: int, classes: int) -> _FrechetArgs:
    a = _FrechetArgs()
    a.n, a.m, a.frames, a.diff = int(n), int(m), int(frames), int(bool(diff))
    a.d_outer, a.d_inner, a.classes = int(d_outer), int(d_inner), int(classes)
    return a


def frechet_workspace_bytes(n: int, m: int, frames: int, diff: bool, d_outer: int, d_inner: int, classes: int) -> int:
    """kg_frechet_workspace_bytes of a shape (RuntimeError naming the field for a shape kg_frechet rejects); no GPU call"""
    return _query("kg_frechet_workspace_bytes", _frechet_shape(n, m, frames, diff, d_outer, d_inner, classes))


def frechet(real: FrechetView, fake: FrechetView, n: int, m: int, frames: int, diff: bool, d_outer: int, d_inner: int,
            classes: int, want_mean: bool = True, moments: bool = False, ws: Optional[torch.Tensor] = None) -> dict:
    """Enqueue kg_frechet (moments, merge, solve and mean launch) on the current stream; no host synchronisation.
    Returns dict(values (classes,) fp64, terms (classes, 4) fp64: |dmu|^2, tr S_r, tr S_f, T, sweeps (classes, 2) int32,
    mean () fp64 or None) on the device; with ``moments`` also mu_real, mu_fake (classes, d) and cov_real, cov_fake
    (classes, d, d) fp64.  ``ws``: a caller's contiguous float64 workspace of at least the needed bytes (its contents do
    not matter), else one is taken with torch.empty."""
    lib = load_library()
    for v in (real, fake):
        if v.t.dtype != torch.float32:
            raise TypeError(f"kg_frechet: fp32 only, got {v.t.dtype}")
    nbytes = frechet_workspace_bytes(n, m, frames, diff, d_outer, d_inner, classes)
    _need_cuda(real.t, fake.t, ws)
    for name, v, cnt in (("real", real, n), ("fake", fake, m)):
        if not _frechet_extent_ok(v, cnt, frames, d_outer, d_inner, classes):
            raise ValueError(f"kg_frechet: the strides of {name} reach outside its tensor")
    dev = real.t.device
    if ws is None:
        ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    elif not ws.is_contiguous() or ws.dtype != torch.float64:
        raise ValueError("kg_frechet: ws must be a contiguous float64 tensor")
    d = d_outer * d_inner
    out = dict(values=torch.empty(classes, dtype=torch.float64, device=dev),
               terms=torch.empty((classes, 4), dtype=torch.float64, device=dev),
               sweeps=torch.empty((classes, 2), dtype=torch.int32, device=dev),
               mean=torch.empty((), dtype=torch.float64, device=dev) if want_mean else None)
    if moments:
        out.update(mu_real=torch.empty((classes, d), dtype=torch.float64, device=dev),
                   mu_fake=torch.empty((classes, d), dtype=torch.float64, device=dev),
                   cov_real=torch.empty((classes, d, d), dtype=torch.float64, device=dev),
                   cov_fake=torch.empty((classes, d, d), dtype=torch.float64, device=dev))
    a = _frechet_shape(n, m, frames, diff, d_outer, d_inner, classes)
    a.real, a.r_sc, a.r_ss, a.r_sf, a.r_so = real.t.data_ptr(), real.sc, real.ss, real.sf, real.so
    a.fake, a.f_sc, a.f_ss, a.f_sf, a.f_so = fake.t.data_ptr(), fake.sc, fake.ss, fake.sf, fake.so
    a.values, a.terms, a.sweeps, a.mean = out["values"].data_ptr(), out["terms"].data_ptr(), out["sweeps"].data_ptr(), \
        _ptr(out["mean"])
    a.mu_real, a.mu_fake = _ptr(out.get("mu_real")), _ptr(out.get("mu_fake"))
    a.cov_real, a.cov_fake = _ptr(out.get("cov_real")), _ptr(out.get("cov_fake"))
    a.ws, a.ws_bytes = ws.data_ptr(), ws.numel() * 8
    pts = (n + m) * (frames - int(bool(diff)))
    _count("kg_frechet", 2.0 * float(pts) * d * d * classes)
    _check(lib.kg_frechet(C.byref(a), _stream()), "kg_frechet")
    return out


def _frechet_real_shape(n: int, frames: int, diff: bool, d_outer: int, d_inner: int, classes: int) -> _FrechetRealArgs:
    a = _FrechetRealArgs()
    a.n, a.frames, a.diff = int(n), int(frames), int(bool(diff))
    a.d_outer, a.d_inner, a.classes = int(d_outer), int(d_inner), int(classes)
    return a


def frechet_real_workspace_bytes(n: int, frames: int, diff: bool, d_outer: int, d_inner: int, classes: int) -> int:
    """kg_frechet_real_workspace_bytes of a shape = 8 classes (nch_r + 1) (d + d*d) (RuntimeError naming the field for a
    shape kg_frechet_real rejects); no GPU call"""
    return _query("kg_frechet_real_workspace_bytes", _frechet_real_shape(n, frames, diff, d_outer, d_inner, classes))


def frechet_real(view: FrechetView, n: int, frames: int, diff: bool, d_outer: int, d_inner: int, classes: int,
                 ws: Optional[torch.Tensor] = None) -> dict:
    """Enqueue kg_frechet_real: the real side of one (data, diff) pair, once (moments, merge and one Jacobi solve with
    vectors per class; three launches, no host synchronisation).  Returns the cache ``frechet_sets`` reads, a dict of
    device tensors: mu_real (classes, d), tr_real (classes), G (classes, e, e) fp64 with e = d + (d & 1), sweeps_real
    (classes) int32 - the bits ``frechet`` forms internally for the same real set."""
    if view.t.dtype != torch.float32:
        raise TypeError(f"kg_frechet_real: fp32 only, got {view.t.dtype}")
    nbytes = frechet_real_workspace_bytes(n, frames, diff, d_outer, d_inner, classes)
    _need_cuda(view.t, ws)
    if not _frechet_extent_ok(view, n, frames, d_outer, d_inner, classes):
        raise ValueError("kg_frechet_real: the strides of real reach outside its tensor")
    dev = view.t.device
    if ws is None:
        ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    elif not ws.is_contiguous() or ws.dtype != torch.float64:
        raise ValueError("kg_frechet_real: ws must be a contiguous float64 tensor")
    d = d_outer * d_inner
    e = d + (d & 1)
    out = dict(mu_real=torch.empty((classes, d), dtype=torch.float64, device=dev),
               tr_real=torch.empty(classes, dtype=torch.float64, device=dev),
               G=torch.empty((classes, e, e), dtype=torch.float64, device=dev),
               sweeps_real=torch.empty(classes, dtype=torch.int32, device=dev))
    a = _frechet_real_shape(n, frames, diff, d_outer, d_inner, classes)
    a.real, a.r_sc, a.r_ss, a.r_sf, a.r_so = view.t.data_ptr(), view.sc, view.ss, view.sf, view.so
    a.mu_real, a.tr_real, a.G, a.sweeps_real = (out[k].data_ptr() for k in ("mu_real", "tr_real", "G", "sweeps_real"))
    a.ws, a.ws_bytes = ws.data_ptr(), ws.numel() * 8
    _count("kg_frechet_real", 2.0 * float(n * (frames - int(bool(diff)))) * d * d * classes)
    _check(load_library().kg_frechet_real(C.byref(a), _stream()), "kg_frechet_real")
    return out


def _frechet_sets_shape(nsets: int, m: int, frames: int, diff: bool, d_outer: int, d_inner: int, classes: int) -> _FrechetSetsArgs:
    a = _FrechetSetsArgs()
    a.nsets, a.m, a.frames, a.diff = int(nsets), int(m), int(frames), int(bool(diff))
    a.d_outer, a.d_inner, a.classes = int(d_outer), int(d_inner), int(classes)
    return a


def frechet_sets_workspace_bytes(nsets: int, m: int, frames: int, diff: bool, d_outer: int, d_inner: int, classes: int) -> int:
    """kg_frechet_sets_workspace_bytes of a shape = 8 nsets classes (nch_f + 1) (d + d*d) (RuntimeError naming the field
    for a shape kg_frechet_sets rejects); no GPU call"""
    return _query("kg_frechet_sets_workspace_bytes", _frechet_sets_shape(nsets, m, frames, diff, d_outer, d_inner, classes))


def frechet_sets(cache: dict, fakes: Sequence[torch.Tensor], f_sc: int, f_ss: int, f_sf: int, f_so: int, m: int, frames: int,
                 diff: bool, d_outer: int, d_inner: int, classes: int, ws: Optional[torch.Tensor] = None) -> dict:
    """Enqueue kg_frechet_sets: the ``fakes`` (1..FRECHET_MAX_SETS fp32 tensors walked with the shared strides f_sc / f_ss /
    f_sf / f_so) against the ``cache`` of ``frechet_real`` for the same frames, diff, d and classes; four launches whatever
    the number of sets, no host synchronisation, the real data is not read.  Returns dict(values (nsets, classes), terms
    (nsets, classes, 4), mean (nsets) fp64, sweeps (nsets, classes) int32, mean32 (nsets) fp32) on the device; every entry
    of set g equals, bit for bit, that of ``frechet(real, fakes[g])`` (sweeps: its column 1).  ``ws`` as in ``frechet``."""
    lib = load_library()
    fakes = list(fakes)
    for t in fakes:
        if t.dtype != torch.float32:
            raise TypeError(f"kg_frechet_sets: fp32 only, got {t.dtype}")
    nsets = len(fakes)
    nbytes = frechet_sets_workspace_bytes(nsets, m, frames, diff, d_outer, d_inner, classes)
    d = d_outer * d_inner
    e = d + (d & 1)
    mu_real, tr_real, G = cache["mu_real"], cache["tr_real"], cache["G"]
    _need_cuda(mu_real, tr_real, G, ws, *fakes)
    for g, t in enumerate(fakes):
        if not _frechet_extent_ok(FrechetView(t, f_sc, f_ss, f_sf, f_so), m, frames, d_outer, d_inner, classes):
            raise ValueError(f"kg_frechet_sets: the strides of fake set {g} reach outside its tensor")
    for name, t, cnt in (("mu_real", mu_real, classes * d), ("tr_real", tr_real, classes), ("G", G, classes * e * e)):
        if t.dtype != torch.float64 or not t.is_contiguous() or t.numel() != cnt:
            raise ValueError(f"kg_frechet_sets: cache entry {name} must be a contiguous float64 tensor of {cnt} elements")
    dev = fakes[0].device
    if ws is None:
        ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    elif not ws.is_contiguous() or ws.dtype != torch.float64:
        raise ValueError("kg_frechet_sets: ws must be a contiguous float64 tensor")
    out = dict(values=torch.empty((nsets, classes), dtype=torch.float64, device=dev),
               terms=torch.empty((nsets, classes, 4), dtype=torch.float64, device=dev),
               sweeps=torch.empty((nsets, classes), dtype=torch.int32, device=dev),
               mean=torch.empty(nsets, dtype=torch.float64, device=dev),
               mean32=torch.empty(nsets, dtype=torch.float32, device=dev))
    a = _frechet_sets_shape(nsets, m, frames, diff, d_outer, d_inner, classes)
    for g, t in enumerate(fakes):
        a.fake[g] = t.data_ptr()
    a.f_sc, a.f_ss, a.f_sf, a.f_so = int(f_sc), int(f_ss), int(f_sf), int(f_so)
    a.mu_real, a.tr_real, a.G = mu_real.data_ptr(), tr_real.data_ptr(), G.data_ptr()
    a.values, a.terms, a.sweeps = out["values"].data_ptr(), out["terms"].data_ptr(), out["sweeps"].data_ptr()
    a.mean, a.mean32 = out["mean"].data_ptr(), out["mean32"].data_ptr()
    a.ws, a.ws_bytes = ws.data_ptr(), ws.numel() * 8
    _count("kg_frechet_sets", 2.0 * nsets * float(m * (frames - int(bool(diff)))) * d * d * classes)
    _check(lib.kg_frechet_sets(C.byref(a), _stream()), "kg_frechet_sets")
    return out


# ---- kinematic plausibility: descriptors and their W1 scores (kg_kin.hip) -----------------------------------

KinView = FrechetView       # element (class c, sample i, frame f, channel o, joint e): the same walk, so = the channel stride


def _kin_table(pairs, what: str):
    """(count, host int32 array or None) of a (count, 2) table of index pairs; the library checks the values"""
    flat = [] if pairs is None else [int(v) for p in pairs for v in p]
    if pairs is not None and any(len(p) != 2 for p in pairs):
        raise ValueError(f"kg_kin_desc: {what} must be (count, 2) index pairs")
    return len(flat) // 2, ((C.c_int32 * len(flat))(*flat) if flat else None)


def _kin_desc_shape(n: int, T: int, Cc: int, V: int, classes: int, bones, mirror, still_eps: float, struct=None):
    """the struct (``_KinDescArgs``, or ``struct``) with everything but the device pointers, and the host tables it points to
    (hold them until the call)"""
    a = (struct or _KinDescArgs)()
    a.n, a.T, a.C, a.V, a.classes = int(n), int(T), int(Cc), int(V), int(classes)
    a.B, tb = _kin_table(bones, "bones")
    a.M, tm = _kin_table(mirror, "mirror")
    a.bones = C.cast(tb, C.c_void_p) if tb is not None else None
    a.mirror = C.cast(tm, C.c_void_p) if tm is not None else None
    a.still_eps = float(still_eps)
    return a, (tb, tm)


def kin_desc_lds_bytes(n: int, T: int, Cc: int, V: int, classes: int, bones, mirror, still_eps: float = 1e-3) -> int:
    """kg_kin_desc_lds_bytes of a shape (RuntimeError naming the field for arguments kg_kin_desc rejects); no GPU call"""
    a, keep = _kin_desc_shape(n, T, Cc, V, classes, bones, mirror, still_eps)
    return _query("kg_kin_desc_lds_bytes", a)


def kin_desc(view: FrechetView, n: int, T: int, Cc: int, V: int, classes: int, bones, mirror, still_eps: float = 1e-3,
             out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Enqueue kg_kin_desc (ONE launch, a workgroup per sample) on the current stream; no host synchronisation.
    ``view`` walks the set as ``FrechetView`` does (so: the channel stride); ``bones`` (B, 2) joint pairs and ``mirror``
    (M, 2) pairs of bone indices are host sequences.  Returns (desc (classes, n, 6) fp32 - ``out`` if given -, degenerate
    (classes,) int32) on the device."""
    who = "kg_kin_desc"
    if view.t.dtype != torch.float32:
        raise TypeError(f"{who}: fp32 only, got {view.t.dtype}")
    a, keep = _kin_desc_shape(n, T, Cc, V, classes, bones, mirror, still_eps)
    nbytes = _query("kg_kin_desc_workspace_bytes", a)
    _need_cuda(view.t, out)
    if not _frechet_extent_ok(view, n, T, Cc, V, classes):
        raise ValueError(f"{who}: the strides of x reach outside its tensor")
    dev = view.t.device
    if out is None:
        out = torch.empty((classes, n, KIN_DESC), dtype=torch.float32, device=dev)
    else:
        _dest(out, classes * n * KIN_DESC, f"{who}: out must be a contiguous fp32 tensor of classes * n * 6 elements")
    degenerate = torch.empty(classes, dtype=torch.int32, device=dev)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    sync = _sync_buffer(dev)
    a.x, a.sc, a.ss, a.sf, a.so = view.t.data_ptr(), view.sc, view.ss, view.sf, view.so
    a.desc, a.degenerate = out.data_ptr(), degenerate.data_ptr()
    a.ws, a.ws_bytes, a.counters, a.counters_len = ws.data_ptr(), nbytes, sync.data_ptr(), sync.numel()
    _count(who, 0.0)
    _check(load_library().kg_kin_desc(C.byref(a), _stream()), who)
    return out, degenerate


def _kin_desc_sets_shape(nsets: int, n: int, T: int, Cc: int, V: int, classes: int, bones, mirror, still_eps: float):
    a, keep = _kin_desc_shape(n, T, Cc, V, classes, bones, mirror, still_eps, struct=_KinDescSetsArgs)
    a.nsets = int(nsets)
    return a, keep


def kin_desc_sets_workspace_bytes(nsets: int, n: int, T: int, Cc: int, V: int, classes: int, bones, mirror,
                                  still_eps: float = 1e-3) -> int:
    """kg_kin_desc_sets_workspace_bytes of a shape (RuntimeError naming the field for arguments it rejects); no GPU call"""
    a, keep = _kin_desc_sets_shape(nsets, n, T, Cc, V, classes, bones, mirror, still_eps)
    return _query("kg_kin_desc_sets_workspace_bytes", a)


def kin_desc_sets_lds_bytes(nsets: int, n: int, T: int, Cc: int, V: int, classes: int, bones, mirror,
                            still_eps: float = 1e-3) -> int:
    """kg_kin_desc_sets_lds_bytes of a shape (RuntimeError naming the field for arguments it rejects); no GPU call"""
    a, keep = _kin_desc_sets_shape(nsets, n, T, Cc, V, classes, bones, mirror, still_eps)
    return _query("kg_kin_desc_sets_lds_bytes", a)


def kin_desc_sets(xs, sc: int, ss: int, sf: int, so: int, n: int, T: int, Cc: int, V: int, classes: int, bones, mirror,
                  still_eps: float = 1e-3, out: Optional[torch.Tensor] = None,
                  ws: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Enqueue kg_kin_desc_sets (ONE launch, a workgroup per (set, class, sample)) on the current stream; no host
    synchronisation.  ``xs``: 1..KIN_MAX_SETS fp32 tensors - or ``FrechetView``s, whose strides must then agree and replace
    the four given - each walked from its first element with the SHARED strides (sc, ss, sf, so: class, sample, frame,
    channel; the joint axis is contiguous).  ``bones`` / ``mirror`` as in ``kin_desc``.  ``ws``: a contiguous fp32 tensor of
    at least ``kin_desc_sets_workspace_bytes`` (default: allocated here).  Returns (desc (nsets, classes, n, 6) fp32 - ``out``
    if given -, degenerate (nsets, classes) int32) on the device; desc[g] and degenerate[g] are bit for bit what ``kin_desc``
    of set g gives."""
    who = "kg_kin_desc_sets"
    xs = list(xs)
    if xs and isinstance(xs[0], FrechetView):
        sc, ss, sf, so = xs[0].sc, xs[0].ss, xs[0].sf, xs[0].so
        if any((v.sc, v.ss, v.sf, v.so) != (sc, ss, sf, so) for v in xs):
            raise ValueError(f"{who}: the sets' views differ in their strides")
        xs = [v.t for v in xs]
    nsets = len(xs)
    for t in xs:
        if t.dtype != torch.float32:
            raise TypeError(f"{who}: fp32 only, got {t.dtype}")
    a, keep = _kin_desc_sets_shape(nsets, n, T, Cc, V, classes, bones, mirror, still_eps)
    nbytes = _query("kg_kin_desc_sets_workspace_bytes", a)
    _need_cuda(*xs, out, ws)
    for g, t in enumerate(xs):
        if not _frechet_extent_ok(FrechetView(t, int(sc), int(ss), int(sf), int(so)), n, T, Cc, V, classes):
            raise ValueError(f"{who}: the strides reach outside the tensor of x[{g}]")
    dev = xs[0].device
    if out is None:
        out = torch.empty((nsets, classes, n, KIN_DESC), dtype=torch.float32, device=dev)
    else:
        _dest(out, nsets * classes * n * KIN_DESC, f"{who}: out must be a contiguous fp32 tensor of nsets * classes * n * 6 elements")
    if ws is None:
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    elif ws.dtype != torch.float32 or not ws.is_contiguous():
        raise ValueError(f"{who}: ws must be a contiguous fp32 tensor")
    degenerate = torch.empty((nsets, classes), dtype=torch.int32, device=dev)
    sync = _sync_buffer(dev)
    per = classes * n * KIN_DESC
    flat = out.view(-1)
    for g, t in enumerate(xs):
        a.x[g] = t.data_ptr()
        a.desc[g] = flat[g * per:(g + 1) * per].data_ptr()
    a.sc, a.ss, a.sf, a.so = int(sc), int(ss), int(sf), int(so)
    a.degenerate = degenerate.data_ptr()
    a.ws, a.ws_bytes, a.counters, a.counters_len = ws.data_ptr(), ws.numel() * 4, sync.data_ptr(), sync.numel()
    _count(who, 0.0)
    _check(load_library().kg_kin_desc_sets(C.byref(a), _stream()), who)
    return out.view(nsets, classes, n, KIN_DESC), degenerate


def _kin_scores_shape(nsets: int, n: int, m: int, classes: int) -> _KinScoresArgs:
    a = _KinScoresArgs()
    a.nsets, a.n, a.m, a.classes = int(nsets), int(n), int(m), int(classes)
    return a


def kin_scores_lds_bytes(nsets: int, n: int, m: int, classes: int) -> int:
    """kg_kin_scores_lds_bytes of a shape (RuntimeError naming the field for a shape kg_kin_scores rejects); no GPU call"""
    return _query("kg_kin_scores_lds_bytes", _kin_scores_shape(nsets, n, m, classes))


def kin_scores(real_desc: torch.Tensor, fake_descs: Sequence[torch.Tensor]) -> dict:
    """Enqueue kg_kin_scores (TWO launches whatever the number of sets): 1..KIN_MAX_SETS fake descriptor matrices (classes,
    m, 6) with a shared m against the real one (classes, n, 6), all contiguous fp32.  Returns device tensors mean_real
    (classes, 6), mean_fake (nsets, classes, 6), w1 (nsets, classes, 6), w1_mean (nsets, 6) fp64, scores (nsets, 6) fp32
    and nonfinite (nsets + 1, classes) int32 (row 0: the real side).  No host synchronisation."""
    who = "kg_kin_scores"
    fake_descs = list(fake_descs)
    nsets = len(fake_descs)
    for name, t in [("real_desc", real_desc)] + [("fake_descs[%d]" % g, t) for g, t in enumerate(fake_descs)]:
        if t.dim() != 3 or t.shape[2] != KIN_DESC or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f"{who}: {name} must be a contiguous fp32 (classes, count, 6) tensor")
        if t.shape[0] != real_desc.shape[0] or (name != "real_desc" and t.shape[1] != fake_descs[0].shape[1]):
            raise ValueError(f"{who}: {name} has shape {tuple(t.shape)}: the sets share classes and m")
    classes, n = real_desc.shape[0], real_desc.shape[1]
    m = fake_descs[0].shape[1] if nsets else 0
    a = _kin_scores_shape(nsets, n, m, classes)
    _query("kg_kin_scores_lds_bytes", a)
    _need_cuda(real_desc, *fake_descs)
    dev = real_desc.device
    out = dict(mean_real=torch.empty((classes, KIN_DESC), dtype=torch.float64, device=dev),
               mean_fake=torch.empty((nsets, classes, KIN_DESC), dtype=torch.float64, device=dev),
               w1=torch.empty((nsets, classes, KIN_DESC), dtype=torch.float64, device=dev),
               w1_mean=torch.empty((nsets, KIN_DESC), dtype=torch.float64, device=dev),
               scores=torch.empty((nsets, KIN_DESC), dtype=torch.float32, device=dev),
               nonfinite=torch.empty((nsets + 1, classes), dtype=torch.int32, device=dev))
    a.real = real_desc.data_ptr()
    for g, t in enumerate(fake_descs):
        a.fake[g] = t.data_ptr()
    a.mean_real, a.mean_fake, a.w1 = out["mean_real"].data_ptr(), out["mean_fake"].data_ptr(), out["w1"].data_ptr()
    a.w1_mean, a.scores, a.nonfinite = out["w1_mean"].data_ptr(), out["scores"].data_ptr(), out["nonfinite"].data_ptr()
    _count(who, 0.0)
    _check(load_library().kg_kin_scores(C.byref(a), _stream()), who)
    return out


# ---- projection into W: per-sample objective and optimiser step (kg_proj.hip) ---------------------------------

def _proj_loss_shape(n: int, Cc: int, T: int, V: int, bones, lambdas, scale: float = 1.0, shift: float = 0.0):
    """a ``_ProjLossArgs`` with everything but the device pointers and strides, and the host table it points to (hold it until
    the call)"""
    a = _ProjLossArgs()
    a.n, a.C, a.T, a.V = int(n), int(Cc), int(T), int(V)
    a.B, tb = _kin_table(bones, "bones")
    a.bones = C.cast(tb, C.c_void_p) if tb is not None else None
    a.lambda_pos, a.lambda_vel, a.lambda_bone = (float(v) for v in lambdas)
    a.scale, a.shift = float(scale), float(shift)
    return a, tb


def _proj_view(who: str, name: str, t: torch.Tensor, shape):
    if t.dtype != torch.float32 or tuple(t.shape) != tuple(shape):
        raise ValueError(f"{who}: {name} must be an fp32 tensor of shape {tuple(shape)}, got {t.dtype} {tuple(t.shape)}")
    if t.shape[3] > 1 and t.stride(3) != 1:
        raise ValueError(f"{who}: the joints of {name} must be contiguous")
    return t.data_ptr(), t.stride(0), t.stride(1), t.stride(2)


def proj_loss(x: torch.Tensor, y: torch.Tensor, bones, lambdas, mask: Optional[torch.Tensor] = None, scale: float = 1.0,
              shift: float = 0.0, loss: Optional[torch.Tensor] = None, gx: Optional[torch.Tensor] = None):
    """Enqueue kg_proj_loss (ONE launch, a workgroup per sample) on the current stream; no host synchronisation.  ``x``, ``y``
    (n, C, T, V) fp32 through strides of their own (joints contiguous), ``y`` read as ``y * scale + shift``; ``mask`` None,
    (T, V) for all samples or (n, T, V), contiguous fp32 weights >= 0; ``bones`` a host sequence of joint pairs (may be
    empty); ``lambdas`` = (pos, vel, bone).  Returns (loss (n, 4) fp32 = [L, L_pos, L_vel, L_bone], gx (n, C, T, V) contiguous
    fp32) - ``loss`` / ``gx`` if given."""
    who = "kg_proj_loss"
    if x.dim() != 4:
        raise ValueError(f"{who}: x must be (n, C, T, V)")
    n, Cc, T, V = x.shape
    a, keep = _proj_loss_shape(n, Cc, T, V, bones, lambdas, scale, shift)
    a.x, a.x_sn, a.x_sc, a.x_st = _proj_view(who, "x", x, x.shape)
    a.y, a.y_sn, a.y_sc, a.y_st = _proj_view(who, "y", y, x.shape)
    if mask is not None:
        if mask.dtype != torch.float32 or not mask.is_contiguous() or tuple(mask.shape) not in ((T, V), (n, T, V)):
            raise ValueError(f"{who}: mask must be a contiguous fp32 tensor of shape (T, V) or (n, T, V), got {tuple(mask.shape)}")
        a.m, a.sm = mask.data_ptr(), (T * V if mask.dim() == 3 else 0)
    _need_cuda(x, y, mask, loss, gx)
    dev = x.device
    if loss is None:
        loss = torch.empty((n, 4), dtype=torch.float32, device=dev)
    else:
        _dest(loss, n * 4, f"{who}: loss must be a contiguous fp32 tensor of n * 4 elements")
    if gx is None:
        gx = torch.empty((n, Cc, T, V), dtype=torch.float32, device=dev)
    else:
        _dest(gx, n * Cc * T * V, f"{who}: gx must be a contiguous fp32 tensor of n * C * T * V elements")
    a.loss, a.gx = loss.data_ptr(), gx.data_ptr()
    _count(who, 0.0)
    _check(load_library().kg_proj_loss(C.byref(a), _stream()), who)
    return loss, gx


def _proj_step_shape(n: int, D: int, K: int, S: int, lr: float, b1: float, b2: float, eps: float, lambda_w: float,
                     ramp_up: int, ramp_down: int) -> _ProjStepArgs:
    a = _ProjStepArgs()
    a.n, a.D, a.K, a.S, a.ramp_up, a.ramp_down = int(n), int(D), int(K), int(S), int(ramp_up), int(ramp_down)
    a.lambda_w, a.lr, a.b1, a.b2, a.eps = float(lambda_w), float(lr), float(b1), float(b2), float(eps)
    return a


def proj_step(w, am, av, gw, wmean, labels, loss, step_t, best_obj, best_loss, best_w, nonfinite, hist, S: int, lr: float,
              b1: float, b2: float, eps: float, lambda_w: float = 0.0, ramp_up: int = 0, ramp_down: int = 0) -> None:
    """Enqueue kg_proj_step (ONE launch, a workgroup per sample) on the current stream: the prior, the schedule, one Adam step
    on the latents ``w`` (n, D) with moments ``am``, ``av`` and the best-so-far record ``best_obj`` (n), ``best_loss`` (n, 4),
    ``best_w`` (n, D); ``hist`` (S, n) or None; ``nonfinite`` (n) int32 counts the steps a sample was frozen.  ``step_t`` holds
    the 1-based number of THIS step (int32, device); the launch does not advance it.  All tensors contiguous."""
    who = "kg_proj_step"
    n, D = w.shape
    K = wmean.shape[0]
    a = _proj_step_shape(n, D, K, S, lr, b1, b2, eps, lambda_w, ramp_up, ramp_down)
    f32 = [("w", w, n * D), ("am", am, n * D), ("av", av, n * D), ("gw", gw, n * D), ("wmean", wmean, K * D), ("loss", loss, n * 4),
           ("best_obj", best_obj, n), ("best_loss", best_loss, n * 4), ("best_w", best_w, n * D)]
    if hist is not None:
        f32.append(("hist", hist, int(S) * n))
    for name, t, cnt in f32:
        _dest(t, cnt, f"{who}: {name} must be a contiguous fp32 tensor of {cnt} elements")
    for name, t, cnt, dt in (("labels", labels, n, torch.int64), ("step", step_t, 1, torch.int32), ("nonfinite", nonfinite, n, torch.int32)):
        if t.dtype != dt or t.numel() != cnt or not t.is_contiguous():
            raise ValueError(f"{who}: {name} must be a contiguous {dt} tensor of {cnt} elements")
    _need_cuda(w, am, av, gw, wmean, labels, loss, step_t, best_obj, best_loss, best_w, nonfinite, hist)
    a.w, a.am, a.av, a.gw, a.wmean = w.data_ptr(), am.data_ptr(), av.data_ptr(), gw.data_ptr(), wmean.data_ptr()
    a.labels, a.loss, a.step = labels.data_ptr(), loss.data_ptr(), step_t.data_ptr()
    a.best_obj, a.best_loss, a.best_w = best_obj.data_ptr(), best_loss.data_ptr(), best_w.data_ptr()
    a.hist, a.nonfinite = _ptr(hist), nonfinite.data_ptr()
    _count(who, 0.0)
    _check(load_library().kg_proj_step(C.byref(a), _stream()), who)


# ---- inputs of a training iteration (kg_input.hip) ------------------------------------------------------------------------

class StepData(NamedTuple):
    """The resident gather of kg_step_inputs: ``data`` (N, C, T, V) fp32 (any strides), ``labels`` (N,) int64,
    ``perm`` (2, perm_stride) int64 (the permutations of the even / odd epochs), outputs ``real`` (B, C, T, V) and
    ``out_labels`` (B,)."""
    data: torch.Tensor
    labels: torch.Tensor
    perm: torch.Tensor
    batches_per_epoch: int
    scale: float
    shift: float
    real: torch.Tensor
    out_labels: torch.Tensor


def noise_views(noise: torch.Tensor, plane_shapes: Sequence[Sequence[int]]):
    """The (critic step, generator step) plane lists inside the flat ``noise`` buffer of kg_step_inputs: plane i of the
    two syntheses are adjacent, so ``torch.cat((d_i, g_i))`` is the memory [2 P_i, 2 P_i + 2 len_i) itself."""
    nd, ng, off = [], [], 0
    for shp in plane_shapes:
        n = 1
        for v in shp:
            n *= int(v)
        nd.append(noise[off:off + n].view(*shp))
        ng.append(noise[off + n:off + 2 * n].view(*shp))
        off += 2 * n
    assert off == noise.numel()
    return nd, ng


def step_inputs(step: torch.Tensor, ticket: torch.Tensor, seed: int, batch_size: int, z: Optional[torch.Tensor] = None,
                alpha: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None,
                plane_len: Sequence[int] = (), gather: Optional[StepData] = None, rank: int = 0, world: int = 1) -> None:
    """Enqueue kg_step_inputs on the current stream: every input of iteration ``step[0]`` (device int64, advanced by the
    launch) - the gathered batch, z (B, latent), alpha (B), the flat injected-noise buffer (``noise_views``)."""
    lib = load_library()
    _need_cuda(step, ticket, z, alpha, noise)
    if step.dtype != torch.int64 or ticket.dtype != torch.int32:
        raise TypeError("kg_step_inputs: step int64 and ticket int32 expected")
    for t in (z, alpha, noise):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise TypeError("kg_step_inputs: contiguous fp32 outputs expected")
    a = _StepInputsArgs()
    a.step, a.ticket, a.seed = step.data_ptr(), ticket.data_ptr(), int(seed) & 0xffffffffffffffff
    a.rank, a.world, a.B = int(rank), int(world), int(batch_size)
    if z is not None:
        if z.dim() != 2 or z.shape[0] != batch_size:
            raise ValueError("kg_step_inputs: z must be (B, latent)")
        a.z, a.latent = z.data_ptr(), z.shape[1]
    if alpha is not None:
        if alpha.numel() != batch_size:
            raise ValueError("kg_step_inputs: alpha must hold B values")
        a.alpha = alpha.data_ptr()
    if noise is not None:
        lens = [int(v) for v in plane_len]
        if not 1 <= len(lens) <= STEP_MAX_PLANES or noise.numel() != 2 * sum(lens):
            raise ValueError("kg_step_inputs: noise must hold 2 * sum(plane_len) values of 1..%d planes" % STEP_MAX_PLANES)
        a.noise, a.n_planes = noise.data_ptr(), len(lens)
        for i, v in enumerate(lens):
            a.plane_len[i] = v
    if gather is not None:
        g = gather
        _need_cuda(g.data, g.labels, g.perm, g.real, g.out_labels)
        if g.data.dtype != torch.float32 or g.data.dim() != 4 or g.real.dtype != torch.float32 or not g.real.is_contiguous():
            raise TypeError("kg_step_inputs: data (N, C, T, V) fp32 and a contiguous fp32 batch expected")
        for t in (g.labels, g.perm, g.out_labels):
            if t.dtype != torch.int64 or not t.is_contiguous():
                raise TypeError("kg_step_inputs: contiguous int64 labels / perm expected")
        n, c, t_, v = g.data.shape
        need = int(g.batches_per_epoch) * int(world) * int(batch_size)
        if tuple(g.real.shape) != (batch_size, c, t_, v) or g.out_labels.numel() != batch_size or g.labels.numel() != n or \
                g.perm.dim() != 2 or g.perm.shape[0] != 2 or g.perm.shape[1] < need or min(g.data.stride()) < 0:
            raise ValueError("kg_step_inputs: shapes of the gather do not fit together")
        a.data = g.data.data_ptr()
        a.d_sN, a.d_sC, a.d_sT, a.d_sV = g.data.stride()
        a.C, a.T, a.V, a.n_rows = c, t_, v, n
        a.label_src, a.perm, a.perm_stride = g.labels.data_ptr(), g.perm.data_ptr(), g.perm.shape[1]
        a.batches_per_epoch, a.scale, a.shift = int(g.batches_per_epoch), float(g.scale), float(g.shift)
        a.real, a.labels = g.real.data_ptr(), g.out_labels.data_ptr()
    _check(lib.kg_step_inputs(C.byref(a), _stream()), "kg_step_inputs")


def loss_append(ring: torch.Tensor, step: torch.Tensor, d_loss: torch.Tensor, g_loss: Optional[torch.Tensor]) -> None:
    """Enqueue kg_loss_append: (d_loss, g_loss) into slot (step - 1) mod len of ``ring`` (len, 2) fp32."""
    _need_cuda(ring, step, d_loss, g_loss)
    if ring.dtype != torch.float32 or ring.dim() != 2 or ring.shape[1] != 2 or not ring.is_contiguous() or step.dtype != torch.int64:
        raise TypeError("kg_loss_append: ring (len, 2) fp32 and step int64 expected")
    for t in (d_loss, g_loss):
        if t is not None and (t.dtype != torch.float32 or t.numel() != 1):
            raise TypeError("kg_loss_append: one-element fp32 losses expected")
    _check(load_library().kg_loss_append(ring.data_ptr(), ring.shape[0], step.data_ptr(), d_loss.data_ptr(), _ptr(g_loss),
                                         _stream()), "kg_loss_append")


# ---- inference-only generation path (kg_sample.hip, kg_genblock.hip, kg_input.hip; sample.Sampler) -----------------------

def bn_eval_coef(jobs: Sequence[dict]) -> None:
    """Eval-mode BatchNorm coefficients of up to BN_EVAL_MAX_JOBS layers in ONE launch (kg_bn_eval_coef).  Each job:
    dict(gamma | None, beta | None, running_mean, running_var, eps, coef (4, C) out); coef = [scale, shift, mean, rstd]
    from the running statistics as they are when the launch runs."""
    lib = load_library()
    if not 1 <= len(jobs) <= BN_EVAL_MAX_JOBS:
        raise ValueError("bn_eval_coef: 1..%d jobs expected" % BN_EVAL_MAX_JOBS)
    arr = (_BnEvalJob * len(jobs))()
    for i, j in enumerate(jobs):
        coef = j["coef"]
        if coef.dim() != 2 or coef.shape[0] != 4 or not coef.is_contiguous() or coef.dtype != torch.float32:
            raise ValueError("bn_eval_coef: coef must be a contiguous fp32 (4, C) tensor")
        c = coef.shape[1]
        vecs = [_vec(j.get(k), c, "bn_eval_coef") for k in ("gamma", "beta", "running_mean", "running_var")]
        if vecs[2] is None or vecs[3] is None:
            raise ValueError("bn_eval_coef: a layer without running statistics has no eval-mode coefficients")
        _need_cuda(coef, *vecs)
        e = arr[i]
        e.C, e.eps, e.coef = c, float(j["eps"]), coef.data_ptr()
        e.gamma, e.beta, e.running_mean, e.running_var = [_ptr(q) for q in vecs]
    _check(lib.kg_bn_eval_coef(arr, len(jobs), _stream()), "kg_bn_eval_coef")


def _gb_infer_dims(a, d: GenBlockDims, slope):
    a.Cin, a.C, a.K, a.Kp, a.Tc, a.Vc, a.T, a.V, a.rep = d.Cin, d.C, d.K, d.Kp, d.Tc, d.Vc, d.T, d.V, d.rep
    a.res_kind, a.act, a.slope = d.res_kind, d.act, slope


def genblock_infer_supported(d: GenBlockDims, n: int, wg, wr, wt) -> bool:
    """Can kg_genblock_infer run this block (the rule of the training forward: genblock_supported)?"""
    a = _GenBlockInferArgs()
    a.N = n
    _gb_infer_dims(a, d, 0.2)
    a.wg, a.wr, a.wt = wg.data_ptr(), _ptr(wr), wt.data_ptr()
    return load_library().kg_genblock_infer_lds_bytes(C.byref(a)) >= 0


def genblock_infer(d: GenBlockDims, *, x, wg, wr=None, br=None, wt, bt=None, B, U=None, ct=None, cr=None, noise=None, nw=None,
                   slope: float = 0.2, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One generator block in eval mode as ONE launch (kg_genblock_infer): x (N, Cin, Tc, Vc) -> out (N, C, T, V) =
    act(u * ct[0] + ct[1] + r * cr[0] + cr[1] + nw * noise), ct / cr the (4, C) coefficients of bn_eval_coef (None: no
    BatchNorm on that branch)."""
    lib = load_library()
    a = _GenBlockInferArgs()
    _gb_infer_dims(a, d, slope)
    x = as_plane(x)
    n, dev = x.shape[0], x.device
    if tuple(x.shape[1:]) != (d.Cin, d.Tc, d.Vc):
        raise ValueError("genblock_infer: input %s does not match (%d, %d, %d)" % (tuple(x.shape), d.Cin, d.Tc, d.Vc))
    a.N, a.x = n, _plane(x)
    _gb_weights(a, wg, wr, wt, B, U)
    a.br, a.bt = _ptr(br), _ptr(bt)
    for name, cf in (("ct", ct), ("cr", cr)):
        if cf is not None and (tuple(cf.shape) != (4, d.C) or not cf.is_contiguous() or cf.dtype != torch.float32):
            raise ValueError("genblock_infer: %s must be a contiguous fp32 (4, C) tensor" % name)
    a.coef_t, a.coef_r = _ptr(ct), _ptr(cr)
    if noise is not None and nw is not None:
        noise, nw = noise.contiguous(), nw.reshape(-1).contiguous()
        if noise.numel() != n * d.T * d.V or nw.numel() != d.C:
            raise ValueError("genblock_infer: noise (N, 1, T, V) and nw (C) expected")
        a.noise, a.nw = noise.data_ptr(), nw.data_ptr()
    else:
        noise = nw = None
    if out is None:
        out = new_plane(n, d.C, d.T, d.V, dev)
    elif tuple(out.shape) != (n, d.C, d.T, d.V):
        raise ValueError("genblock_infer: out must be (N, C, T, V)")
    a.out = _plane(out)
    _need_cuda(x, wg, wr, br, wt, bt, B, U, ct, cr, noise, nw, out)
    Mh = d.Kp * d.C + (d.C if d.res_kind == 2 else 0)
    _count("kg_genblock", 2.0 * n * (Mh * d.Cin * d.Tc * d.Vc + 3 * d.C * d.C * d.T * d.V) +
           2.0 * n * (d.Kp + (1 if d.res_kind else 0)) * d.Vc * d.V * d.C * d.Tc)
    _gb_record_form(d, n, "infer", a)
    _check(lib.kg_genblock_infer(C.byref(a), _stream()), "kg_genblock_infer")
    return out


def sample_inputs(step: torch.Tensor, ticket: torch.Tensor, seed: int, z: Optional[torch.Tensor] = None,
                  noise: Optional[torch.Tensor] = None, t: Optional[torch.Tensor] = None) -> None:
    """Enqueue kg_sample_inputs: the random inputs of replay ``step[0]`` (device int64, advanced by the launch) - z
    (B, latent), the flat noise buffer of one synthesis, the truncation draws t (mean_size, Dt); None = not drawn."""
    _need_cuda(step, ticket, z, noise, t)
    if step.dtype != torch.int64 or ticket.dtype != torch.int32:
        raise TypeError("kg_sample_inputs: step int64 and ticket int32 expected")
    for q in (z, noise, t):
        if q is not None and (q.dtype != torch.float32 or not q.is_contiguous()):
            raise TypeError("kg_sample_inputs: contiguous fp32 outputs expected")
    a = _SampleInputsArgs()
    a.step, a.ticket, a.seed = step.data_ptr(), ticket.data_ptr(), int(seed) & 0xffffffffffffffff
    if z is not None:
        if z.dim() != 2:
            raise ValueError("kg_sample_inputs: z must be (B, latent)")
        a.z, a.B, a.latent = z.data_ptr(), z.shape[0], z.shape[1]
    if noise is not None:
        a.noise, a.noise_len = noise.data_ptr(), noise.numel()
    if t is not None:
        if t.dim() != 2:
            raise ValueError("kg_sample_inputs: t must be (mean_size, Dt)")
        a.t, a.t_rows, a.t_cols = t.data_ptr(), t.shape[0], t.shape[1]
    _check(load_library().kg_sample_inputs(C.byref(a), _stream()), "kg_sample_inputs")


def trunc_lerp(x: torch.Tensor, t: torch.Tensor, truncation: float) -> torch.Tensor:
    """x (N, D) <- m + truncation * (x - m) in place, m = column means of t (M, D) (kg_trunc_lerp); returns x."""
    _need_cuda(x, t)
    for q in (x, t):
        if q.dim() != 2 or q.dtype != torch.float32 or q.stride(1) != 1:
            raise TypeError("kg_trunc_lerp: fp32 (rows, D) matrices with unit column stride expected")
    if x.shape[1] != t.shape[1]:
        raise ValueError("kg_trunc_lerp: x (N, %d) and t (M, %d) differ in D" % (x.shape[1], t.shape[1]))
    _check(load_library().kg_trunc_lerp(x.data_ptr(), x.stride(0), x.shape[0], x.shape[1], t.data_ptr(), t.stride(0), t.shape[0],
                                        float(truncation), _stream()), "kg_trunc_lerp")
    return x


# ---- scoring during training (kg_eval.hip; evaluate.Evaluator) --------------------------------------------------------------

def _eval_record(struct, most: int, who: str, scores, select, iteration, count, ring_val, ring_iter, best_val, best_iter, flag,
                 maximise=None):
    """``eval_record`` / ``eval_record2`` / ``eval_record3``: the tensor checks, the fill of an instance of ``struct`` (room
    for ``most`` scores; ``maximise``: None when it has no such field) and the launch; ``who`` is the entry point's name."""
    _need_cuda(iteration, count, ring_val, ring_iter, best_val, best_iter, flag, *scores)
    for t in scores:
        if t.dtype != torch.float32 or t.numel() != 1:
            raise TypeError("%s: one-element fp32 scores expected" % who)
    for t in (iteration, count, best_iter):
        if t is not None and (t.dtype != torch.int64 or t.numel() != 1):
            raise TypeError("%s: one-element int64 iteration / count / best_iter expected" % who)
    if best_val.dtype != torch.float32 or best_val.numel() != 1 or flag.dtype != torch.int32 or flag.numel() != 1:
        raise TypeError("%s: one-element fp32 best_val and int32 flag expected" % who)
    if ring_val.dtype != torch.float32 or ring_iter.dtype != torch.int64 or not ring_val.is_contiguous() or \
            not ring_iter.is_contiguous():
        raise TypeError("%s: contiguous ring_val fp32 and ring_iter int64 expected" % who)
    n = len(scores)
    ring_len = ring_val.shape[0] if ring_val.dim() == 2 else 0
    if ring_val.dim() != 2 or ring_iter.dim() != 2 or (ring_len and (ring_val.shape[1] != n or tuple(ring_iter.shape) != (ring_len, 2))):
        raise ValueError("%s: ring_val (len, nscores) and ring_iter (len, 2) expected" % who)
    a = struct()
    for i, t in enumerate(scores[:most]):   # (more than fit: the library names nscores)
        a.scores[i] = t.data_ptr()
    a.nscores, a.select, a.ring_len = n, int(select), ring_len
    a.iter, a.count = _ptr(iteration), count.data_ptr()
    a.ring_val, a.ring_iter = ring_val.data_ptr(), ring_iter.data_ptr()
    a.best_val, a.best_iter, a.flag = best_val.data_ptr(), best_iter.data_ptr(), flag.data_ptr()
    if maximise is not None:
        a.maximise = 1 if maximise else 0
    _check(getattr(load_library(), who)(C.byref(a), _stream()), who)


def eval_record(scores: Sequence[torch.Tensor], select: int, iteration: Optional[torch.Tensor], count: torch.Tensor,
                ring_val: torch.Tensor, ring_iter: torch.Tensor, best_val: torch.Tensor, best_iter: torch.Tensor,
                flag: torch.Tensor) -> None:
    """Enqueue kg_eval_record: the one-element fp32 ``scores`` of an evaluation into slot ``count mod len`` of ``ring_val``
    (len, nscores) fp32 and ``ring_iter`` (len, 2) int64 = [iteration, improved]; ``flag`` (int32) = scores[select] <
    best_val (strict), and then best_val / best_iter (int64) take the score and ``iteration[0]`` (int64; None: -1);
    ``count`` (int64) is advanced."""
    _eval_record(_EvalRecordArgs, EVAL_MAX_SCORES, "kg_eval_record", scores, select, iteration, count, ring_val, ring_iter,
                 best_val, best_iter, flag)


def eval_record2(scores: Sequence[torch.Tensor], select: int, iteration: Optional[torch.Tensor], count: torch.Tensor,
                 ring_val: torch.Tensor, ring_iter: torch.Tensor, best_val: torch.Tensor, best_iter: torch.Tensor,
                 flag: torch.Tensor, maximise: bool = False) -> None:
    """Enqueue kg_eval_record2: ``eval_record`` for up to EVAL2_MAX_SCORES scores and with a sense - ``maximise``: ``flag``
    = scores[select] > best_val (strict; the host starts best_val at -inf), else scores[select] < best_val."""
    _eval_record(_EvalRecord2Args, EVAL2_MAX_SCORES, "kg_eval_record2", scores, select, iteration, count, ring_val, ring_iter,
                 best_val, best_iter, flag, bool(maximise))


def eval_record3(scores: Sequence[torch.Tensor], select: int, iteration: Optional[torch.Tensor], count: torch.Tensor,
                 ring_val: torch.Tensor, ring_iter: torch.Tensor, best_val: torch.Tensor, best_iter: torch.Tensor,
                 flag: torch.Tensor, maximise: bool = False) -> None:
    """Enqueue kg_eval_record3: ``eval_record2`` for up to EVAL3_MAX_SCORES scores (the same kernel template; with 32 scores or
    fewer it leaves the bits of ``eval_record2``)."""
    _eval_record(_EvalRecord3Args, EVAL3_MAX_SCORES, "kg_eval_record3", scores, select, iteration, count, ring_val, ring_iter,
                 best_val, best_iter, flag, bool(maximise))


def copy_if(flag: torch.Tensor, jobs: Sequence[Tuple[torch.Tensor, torch.Tensor]]) -> None:
    """Enqueue kg_copy_if: when ``flag[0]`` (int32, device) is non-zero at the time the launch RUNS, every (src, dst) pair -
    contiguous tensors of one dtype and size, element size a multiple of 4 bytes - is copied bit for bit; otherwise nothing
    is written.  COPY_IF_MAX_JOBS pairs per launch, more pairs take more launches."""
    if flag.dtype != torch.int32 or flag.numel() != 1:
        raise TypeError("kg_copy_if: one-element int32 flag expected")
    _need_cuda(flag)
    lib = load_library()
    jobs = list(jobs)
    for part in _chunks(jobs, COPY_IF_MAX_JOBS):
        arr = (_CopyJob * len(part))()
        for i, (src, dst) in enumerate(part):
            _need_cuda(src, dst)
            if src.dtype != dst.dtype or src.element_size() % 4:
                raise TypeError("kg_copy_if: src and dst of one dtype with 4- or 8-byte elements expected (got %s, %s)"
                                % (src.dtype, dst.dtype))
            if src.numel() != dst.numel() or not src.is_contiguous() or not dst.is_contiguous():
                raise ValueError("kg_copy_if: contiguous src and dst of one size expected")
            arr[i].src, arr[i].dst = src.data_ptr(), dst.data_ptr()
            arr[i].nwords = src.numel() * (src.element_size() // 4)
        _count("kg_copy_if", 0.0)
        _check(lib.kg_copy_if(flag.data_ptr(), arr, len(part), _stream()), "kg_copy_if")



class Comm:
    """One RCCL communicator owned through the C ABI (kg_comm_init / kg_allreduce_flat / kg_comm_destroy).
    ``exchange(id_bytes | None) -> id_bytes``: ships rank 0's unique id to every rank (any side channel: a
    torch.distributed object broadcast, a file, an MPI bcast ...).  ``world == 1`` needs no exchange."""

    def __init__(self, rank: int, world: int, device: int, exchange=None):
        lib = load_library()
        buf = C.create_string_buffer(COMM_ID_BYTES)
        if rank == 0:
            _check(lib.kg_comm_unique_id(buf), "kg_comm_unique_id")
        if world > 1:
            if exchange is None:
                raise ValueError("Comm: world > 1 needs an `exchange` callable for the unique id")
            raw = exchange(bytes(buf.raw) if rank == 0 else None)
            if not isinstance(raw, (bytes, bytearray)) or len(raw) != COMM_ID_BYTES:
                raise ValueError("Comm: exchange() must return rank 0's %d id bytes" % COMM_ID_BYTES)
            buf = C.create_string_buffer(bytes(raw), COMM_ID_BYTES)
        self._h = C.c_void_p()
        _check(lib.kg_comm_init(C.byref(self._h), rank, world, buf, device), "kg_comm_init")
        self.rank, self.world, self.device = rank, world, device
        self.force = False      # tests: issue the collective even with one rank (RCCL then copies in place)

    def allreduce_(self, flat: torch.Tensor) -> torch.Tensor:
        """flat <- sum over ranks (in place), enqueued on torch's current stream."""
        if self._h is None:
            raise RuntimeError("Comm: destroyed")
        _need_cuda(flat)
        if flat.dtype != torch.float32 or not flat.is_contiguous():
            raise ValueError("Comm.allreduce_: contiguous fp32 buffer expected")
        _check(load_library().kg_allreduce_flat(self._h, flat.data_ptr(), flat.numel(), _stream()), "kg_allreduce_flat")
        return flat

    def destroy(self):
        if self._h is not None:
            h, self._h = self._h, None
            _check(load_library().kg_comm_destroy(h), "kg_comm_destroy")

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def torch_dist_exchange(src: int = 0):
    """`exchange` callable for Comm over an initialised torch.distributed process group (gloo or nccl)."""
    import torch.distributed as dist

    def ex(raw):
        box = [raw]
        dist.broadcast_object_list(box, src=src)
        return box[0]
    return ex
