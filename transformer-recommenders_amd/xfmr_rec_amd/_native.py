"""ctypes binding of ``libxfmr_hip.so`` (C ABI declared in ``include/xfmr_hip.h``; the Structures and the signature tables
are in ``_abi.py`` and re-exported here).

There is no CPU fallback: every op in this package goes through this library. If the shared object is
missing, cannot be loaded, or a tensor is not on a HIP device, the call raises -- it never silently
computes with PyTorch instead.
"""

from __future__ import annotations

import ctypes as C
import os
import pathlib

import torch

from ._abi import (INTERNAL_SIGNATURES, NOT_BOUND, SEARCH_SIGNATURES, SESSION_SIGNATURES, SIGNATURES, DwItem, EncoderCfg, LnResidual,  # noqa: F401
                   LossCfg, OptCfg, ReduceSeg, Seed, bind)

_HERE = pathlib.Path(__file__).resolve().parent
# XFMR_HIP_LIB points at another build of the same library (kernel experiments); the default is the in-tree one
LIB_PATH = pathlib.Path(os.environ["XFMR_HIP_LIB"]) if os.environ.get("XFMR_HIP_LIB") else _HERE / "libxfmr_hip.so"

PREC_F32, PREC_BF16 = 0, 1
PRECISIONS = {"fp32": PREC_F32, "f32": PREC_F32, "bf16": PREC_BF16}
EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_DROP_RES = 0, 1, 2
NEG_SHARED, NEG_CATALOG = 0, 1
ATTN_CAUSAL, ATTN_BIDIRECTIONAL = 0, 1  # xfmr_attn_{fwd,bwd}_mode
ATTN_STREAM_KEYS = 2  # OR-ed into the attn_mode above: the key-streaming form at any L (generic kernels; bf16 head size 32)
# xfmr_encoder_cfg.flags
ENC_BIDIRECTIONAL, ENC_LN_UNFUSED, ENC_FFN_UNFUSED, ENC_FFN_BWD_UNFUSED, ENC_DW_INLINE, ENC_DW_SIDE_ANY = 1, 2, 4, 8, 16, 32
ENC_DW_UNPAIRED, ENC_REDUCE_HALF_EARLY = 64, 128
LOSS_DTOK_ZEROED = 1  # xfmr_loss_cfg.flags
LOSS_STATS_ELSEWHERE = 2  # ... the call's stats[] are not read: an InfoNCE gradient pass skips its count
ABI_VERSION = 3
ECOMM = -6  # XFMR_ECOMM: RCCL not loadable / an RCCL call failed (xfmr_comm_last_error has RCCL's text)
NUM_LOSSES, NUM_STATS = 7, 16
RANK_NONE = 0x7FFFFFFF  # XFMR_RANK_NONE: a target that is not eligible has no rank
MAX_RANK_CUTOFFS = 8  # cutoffs per xfmr_rank_metrics_sum call
LOSS_IDS = {
    "AlignmentLoss": 0,
    "AlignmentContrastiveLoss": 1,
    "ContrastiveLoss": 2,
    "InfoNCELoss": 3,
    "NCELoss": 4,
    "PairwiseHingeLoss": 5,
    "PairwiseLogisticLoss": 6,
}
STAT = dict(
    n_valid=0, n_query=1, neg_density=2, pos_mean=3, pos_std=4, pos_min=5, pos_max=6,
    neg_mean=7, neg_std=8, neg_min=9, neg_max=10, neg_count=11, neg_distinct=12, pos_density=13, attn_density=14,
)
PROF_FFN_FWD, PROF_FFN_BWD, PROF_ATTN_FWD, PROF_ATTN_BWD, PROF_DW, PROF_REDUCE = 1, 2, 3, 4, 5, 6
CLIP_NONE, CLIP_NORM, CLIP_VALUE = 0, 1, 2  # xfmr_opt_cfg.clip_mode
CLIP_MODES = {None: CLIP_NONE, "none": CLIP_NONE, "norm": CLIP_NORM, "value": CLIP_VALUE}
# xfmr_opt_cfg.sched: a LambdaLR with the lr_lambda of transformers.optimization.get_*_schedule_with_warmup
SCHEDULES = {"constant": 0, "warmup_constant": 1, "warmup_linear": 2, "warmup_cosine": 3}
# the words of the xfmr_opt_ctl record (nonfinite is a uint32: read it through an int32 view)
CTL = dict(grad_norm=0, grad_max_abs=1, clip_coef=2, lr=3, nonfinite=4)
TARGET_FIRST, TARGET_DIAGONAL, TARGET_EXPLICIT = 0, 1, 2
TARGET_MODES = {"first": TARGET_FIRST, "diagonal": TARGET_DIAGONAL, None: TARGET_EXPLICIT}  # LossConfig.target_position
POOL_MODES = {"mean": 0, "max": 1, "cls": 2, "lasttoken": 3}
COMM_ID_BYTES = 128
_SIGNATURES = SIGNATURES
EXPORTED_SYMBOLS = tuple(SIGNATURES)  # the public C ABI
INTERNAL_SYMBOLS = tuple(INTERNAL_SIGNATURES)  # csrc/internal.h: bound for tests and probes, no part of the public ABI
SESSION_SYMBOLS = tuple(SESSION_SIGNATURES)  # include/xfmr_session.h: the session encoder's public entries
SEARCH_SYMBOLS = tuple(SEARCH_SIGNATURES)  # include/xfmr_search.h: the refined item search's public entries

_lib = None


class NativeLibraryError(RuntimeError):
    pass


def load() -> C.CDLL:
    """Load the library once. ``torch`` is imported first so that its bundled HIP runtime
    (same soname ``libamdhip64.so.7``) is the one the library binds to."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise NativeLibraryError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C transformer-recommenders_amd/csrc`). There is no CPU fallback."
        )
    try:
        lib = C.CDLL(str(LIB_PATH), mode=C.RTLD_GLOBAL)
    except OSError as e:  # pragma: no cover - depends on the host
        raise NativeLibraryError(f"cannot load {LIB_PATH}: {e}") from e
    got = lib.xfmr_abi_version() if hasattr(lib, "xfmr_abi_version") else None
    if got != ABI_VERSION:  # checked before binding the symbols: an older build fails here with a version message
        raise NativeLibraryError(f"{LIB_PATH}: ABI version {got}, this package binds version {ABI_VERSION}: rebuild the "
                                 "library (python -c 'import __graft_entry__ as g; g.build()')")
    try:
        _lib = bind(lib)
    except AttributeError as e:
        raise NativeLibraryError(str(e)) from e
    return lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().xfmr_strerror(rc).decode()
        if rc == ECOMM:
            msg += ": " + load().xfmr_comm_last_error().decode()
        raise RuntimeError(f"{what} failed: {msg} (code {rc})")


def ptr(t: torch.Tensor | None) -> int | None:
    """Device pointer of a contiguous HIP tensor (None passes NULL)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError(
            "xfmr_rec_amd ops run only on a HIP device (MI355X); got a CPU tensor. There is no CPU fallback."
        )
    if not t.is_contiguous():
        raise RuntimeError("xfmr_rec_amd ops need contiguous tensors")
    return t.data_ptr()


def stream() -> int:
    """hipStream_t of torch's current stream on the current device. Called once per launch sequence: the raw accessor
    (no ``torch.cuda.Stream`` object, no ``is_available()`` / device-count probe per call: ~10 us each on the host of a
    host-bound small step) where this torch has it."""
    try:
        return torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice())
    except AttributeError:  # pragma: no cover - older / newer torch without the private accessors
        return torch.cuda.current_stream().cuda_stream


def precision_id(p) -> int:
    if isinstance(p, int):
        return p
    try:
        return PRECISIONS[str(p).lower()]
    except KeyError:
        raise ValueError(f"precision must be one of {sorted(PRECISIONS)}; got {p!r}") from None
