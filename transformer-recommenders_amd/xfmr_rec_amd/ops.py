"""Thin functional wrappers over the C ABI + the two autograd Functions of the training path.

Every function here enqueues HIP kernels from ``libxfmr_hip.so`` on the current stream of the current
device. Tensors are allocated with torch (device memory + caching allocator are plumbing); the
arithmetic is never torch's.
"""

from __future__ import annotations

import ctypes as C
import dataclasses
import os

import torch

from . import _native as N

f32 = torch.float32


def _empty(shape, like: torch.Tensor, dtype=f32):
    return torch.empty(shape, dtype=dtype, device=like.device)


def _bytes(n: int, like: torch.Tensor):
    return torch.empty(max(int(n), 16), dtype=torch.uint8, device=like.device)


def selftest_mfma(device="cuda") -> list[int]:
    out = torch.full((4 + 4096,), -1, dtype=torch.int32, device=device)  # 4 result words + 16 KiB scratch
    N.check(N.load().xfmr_selftest_mfma(N.ptr(out), N.stream()), "xfmr_selftest_mfma")
    return out[:4].tolist()


# ------------------------------------------------------------------------------------------------ per-op
def embed_ln_fwd(item_idx, table, pos_emb, type_emb, gamma, beta, *, eps=1e-12, dropout_p=0.0, seed=0, site=0):
    B, L = item_idx.shape
    H = table.shape[1]
    out, pre = _empty((B, L, H), table), _empty((B, L, H), table)
    mean, rstd = _empty((B, L), table), _empty((B, L), table)
    mask = _empty((B, L), table, torch.uint8)
    N.check(
        N.load().xfmr_embed_ln_fwd(
            N.ptr(item_idx), N.ptr(table), table.shape[0], N.ptr(pos_emb), N.ptr(type_emb), N.ptr(gamma),
            N.ptr(beta), N.ptr(out), N.ptr(pre), N.ptr(mean), N.ptr(rstd), N.ptr(mask), B, L, H, eps, dropout_p,
            seed, site, N.stream(),
        ),
        "xfmr_embed_ln_fwd",
    )
    return out, pre, mean, rstd, mask


def embed_param_grads(d_pre, max_pos):
    B, L, H = d_pre.shape
    d_pos, d_type = _empty((max_pos, H), d_pre), _empty((2, H), d_pre)
    N.check(
        N.load().xfmr_embed_param_grads(N.ptr(d_pre), N.ptr(d_pos), N.ptr(d_type), B, L, H, max_pos, N.stream()),
        "xfmr_embed_param_grads",
    )
    return d_pos, d_type


def layernorm_fwd(x, gamma, beta, eps=1e-12):
    rows, H = x.numel() // x.shape[-1], x.shape[-1]
    y, mean, rstd = torch.empty_like(x), _empty((rows,), x), _empty((rows,), x)
    N.check(
        N.load().xfmr_layernorm_fwd(N.ptr(x), N.ptr(gamma), N.ptr(beta), N.ptr(y), N.ptr(mean), N.ptr(rstd), rows, H,
                                    eps, N.stream()),
        "xfmr_layernorm_fwd",
    )
    return y, mean, rstd


def layernorm_bwd(dy, x, mean, rstd, gamma, *, dropout_p=0.0, seed=0, site=0):
    rows, H = x.numel() // x.shape[-1], x.shape[-1]
    lib = N.load()
    dx = torch.empty_like(x)
    d_lin = torch.empty_like(x) if dropout_p > 0 else None
    dg, db, dbias = _empty((H,), x), _empty((H,), x), _empty((H,), x)
    ws = _bytes(lib.xfmr_layernorm_bwd_workspace(rows, H), x)
    N.check(
        lib.xfmr_layernorm_bwd(N.ptr(dy), N.ptr(x), N.ptr(mean), N.ptr(rstd), N.ptr(gamma), N.ptr(dx), N.ptr(d_lin),
                               N.ptr(dg), N.ptr(db), N.ptr(dbias), rows, H, dropout_p, seed, site, N.ptr(ws),
                               N.stream()),
        "xfmr_layernorm_bwd",
    )
    return dx, d_lin, dg, db, dbias


def linear_fwd(x, w, bias, *, epilogue=N.EPI_BIAS, residual=None, dropout_p=0.0, seed=0, site=0, precision="bf16"):
    M, K = x.numel() // x.shape[-1], x.shape[-1]
    Nout = w.shape[0]
    y = _empty((*x.shape[:-1], Nout), x)
    aux = torch.empty_like(y) if epilogue == N.EPI_BIAS_GELU else None
    N.check(
        N.load().xfmr_linear_fwd(N.ptr(x), N.ptr(w), N.ptr(bias), N.ptr(y), M, Nout, K, epilogue, N.ptr(residual),
                                 N.ptr(aux), dropout_p, seed, site, N.precision_id(precision), N.stream()),
        "xfmr_linear_fwd",
    )
    return (y, aux) if aux is not None else y


def linear_bwd_dx(dy, w, *, residual_grad=None, gelu_pre=None, precision="bf16"):
    M, Nout = dy.numel() // dy.shape[-1], dy.shape[-1]
    K = w.shape[1]
    dx = _empty((*dy.shape[:-1], K), dy)
    N.check(
        N.load().xfmr_linear_bwd_dx(N.ptr(dy), N.ptr(w), N.ptr(dx), M, Nout, K, N.ptr(residual_grad),
                                    N.ptr(gelu_pre), N.precision_id(precision), N.stream()),
        "xfmr_linear_bwd_dx",
    )
    return dx


def linear_bwd_dw(dy, x, *, precision="bf16"):
    M, Nout = dy.numel() // dy.shape[-1], dy.shape[-1]
    K = x.shape[-1]
    lib = N.load()
    dw = _empty((Nout, K), dy)
    nbytes = lib.xfmr_linear_bwd_dw_workspace(M, Nout, K)
    ws = _bytes(nbytes, dy)
    N.check(
        lib.xfmr_linear_bwd_dw(N.ptr(dy), N.ptr(x), N.ptr(dw), M, Nout, K, N.precision_id(precision), N.ptr(ws),
                               nbytes, N.stream()),
        "xfmr_linear_bwd_dw",
    )
    return dw


def colsum(a):
    M, Nc = a.numel() // a.shape[-1], a.shape[-1]
    lib = N.load()
    out = _empty((Nc,), a)
    ws = _bytes(lib.xfmr_colsum_workspace(M, Nc), a)
    N.check(lib.xfmr_colsum(N.ptr(a), N.ptr(out), M, Nc, N.ptr(ws), N.stream()), "xfmr_colsum")
    return out


def attn_fwd(qkv, key_mask, heads, *, dropout_p=0.0, seed=0, site=0, precision="bf16", causal=True, stream_keys=False):
    """stream_keys: the key-streaming form even where the whole-panel form fits LDS. Generic kernels (fp32 policy, head
    size 64): bit-identical results. bf16 policy at head size 32: the key-streaming two-kernel form, bit-identical to the
    two-kernel panel form; against the one-workgroup forms (causal, L <= 512) equal within the bf16 tolerance only."""
    B, L, H3 = qkv.shape
    H = H3 // 3
    ctx, lse = _empty((B, L, H), qkv), _empty((B, heads, L), qkv)
    lib = N.load()
    head = (N.ptr(qkv), N.ptr(key_mask), N.ptr(ctx), N.ptr(lse), B, L, heads, H, dropout_p, seed, site,
            N.precision_id(precision))
    if causal and not stream_keys:
        N.check(lib.xfmr_attn_fwd(*head, N.stream()), "xfmr_attn_fwd")
    else:
        mode = (N.ATTN_CAUSAL if causal else N.ATTN_BIDIRECTIONAL) | (N.ATTN_STREAM_KEYS if stream_keys else 0)
        N.check(lib.xfmr_attn_fwd_mode(*head, mode, N.stream()), "xfmr_attn_fwd_mode")
    return ctx, lse


def attn_bwd(qkv, key_mask, ctx, lse, d_ctx, heads, *, dropout_p=0.0, seed=0, site=0, precision="bf16", causal=True,
             stream_keys=False):
    """stream_keys: as attn_fwd -- the key-streaming dQ and dK/dV kernels at any L. In the bf16 policy at head size 32 they
    are bit-identical to the two-kernel panel form, and within the bf16 gradient tolerance of the one-workgroup forms."""
    B, L, H3 = qkv.shape
    d_qkv = torch.empty_like(qkv)
    lib = N.load()
    head = (N.ptr(qkv), N.ptr(key_mask), N.ptr(ctx), N.ptr(lse), N.ptr(d_ctx), N.ptr(d_qkv), B, L, heads, H3 // 3,
            dropout_p, seed, site, N.precision_id(precision))
    if causal and not stream_keys:
        N.check(lib.xfmr_attn_bwd(*head, N.stream()), "xfmr_attn_bwd")
    else:
        mode = (N.ATTN_CAUSAL if causal else N.ATTN_BIDIRECTIONAL) | (N.ATTN_STREAM_KEYS if stream_keys else 0)
        N.check(lib.xfmr_attn_bwd_mode(*head, mode, N.stream()), "xfmr_attn_bwd_mode")
    return d_qkv


def table_rnorm(table):
    out = _empty((table.shape[0],), table)
    N.check(N.load().xfmr_table_rnorm(N.ptr(table), N.ptr(out), table.shape[0], table.shape[1], N.stream()),
            "xfmr_table_rnorm")
    return out


def table_prepare(table):
    """(rnorm, table_bf16): per-item inverse norms + the bf16 gather copy of the frozen table."""
    rn = _empty((table.shape[0],), table)
    tb = torch.empty(table.shape, dtype=torch.bfloat16, device=table.device)
    N.check(N.load().xfmr_table_prepare(N.ptr(table), N.ptr(rn), N.ptr(tb), table.shape[0], table.shape[1],
                                        N.stream()), "xfmr_table_prepare")
    return rn, tb


def mean_pool(tok, key_mask):
    B, L, H = tok.shape
    out = _empty((B, H), tok)
    N.check(N.load().xfmr_mean_pool(N.ptr(tok), N.ptr(key_mask), N.ptr(out), B, L, H, N.stream()), "xfmr_mean_pool")
    return out


def pool(tok, key_mask, mode: str = "mean"):
    """sentence-transformers Pooling(pooling_mode) over (B,L,H) tokens; forward only."""
    if use_torch_ops():
        return torch.ops.xfmr.pool(tok, key_mask, N.POOL_MODES[mode])
    B, L, H = tok.shape
    out = _empty((B, H), tok)
    N.check(N.load().xfmr_pool(N.ptr(tok), N.ptr(key_mask), N.ptr(out), B, L, H, N.POOL_MODES[mode], N.stream()),
            "xfmr_pool")
    return out


def pool_rows(tok, seq_offsets, mode: str = "mean", *, normalize: bool = False, eps: float = 1e-12):
    """:func:`pool` over the PACKED layout: tok (rows, H), seq_offsets (B + 1) int32 on the device (ops.pack_rows's
    ``seq_offsets``); ``normalize`` fuses :func:`l2_normalize`. Returns (B, H); an empty sequence gives a zero row.
    Forward only."""
    B, H = seq_offsets.numel() - 1, tok.shape[-1]
    out = _empty((B, H), tok)
    N.check(N.load().xfmr_pool_rows(N.ptr(tok), N.ptr(seq_offsets), N.ptr(out), B, H, N.POOL_MODES[mode],
                                    int(bool(normalize)), float(eps), N.stream()), "xfmr_pool_rows")
    return out


def table_sqnorm(table):
    """Squared row norms of the item table (the l2 metric's item term of xfmr_topk_tiled)."""
    out = _empty((table.shape[0],), table)
    N.check(N.load().xfmr_table_sqnorm(N.ptr(table), N.ptr(out), table.shape[0], table.shape[1], N.stream()),
            "xfmr_table_sqnorm")
    return out


class L2NormalizeFunction(torch.autograd.Function):
    """``torch.nn.functional.normalize(x, dim=-1)`` (``models.py:393-394``) on (rows, H)."""

    @staticmethod
    def forward(ctx, x, eps=1e-12):
        x = x.contiguous().to(f32)
        rows, H = x.numel() // x.shape[-1], x.shape[-1]
        y, inv = torch.empty_like(x), _empty((rows,), x)
        N.check(N.load().xfmr_l2_normalize_fwd(N.ptr(x), N.ptr(y), N.ptr(inv), rows, H, eps, N.stream()),
                "xfmr_l2_normalize_fwd")
        ctx.save_for_backward(y, inv)
        ctx.eps = eps
        return y

    @staticmethod
    def backward(ctx, dy):
        y, inv = ctx.saved_tensors
        dy = dy.contiguous().to(f32)
        dx = torch.empty_like(y)
        rows, H = y.numel() // y.shape[-1], y.shape[-1]
        N.check(N.load().xfmr_l2_normalize_bwd(N.ptr(dy), N.ptr(y), N.ptr(inv), N.ptr(dx), rows, H, ctx.eps, N.stream()),
                "xfmr_l2_normalize_bwd")
        return dx, None


def l2_normalize(x, eps: float = 1e-12):
    if use_torch_ops():
        return torch.ops.xfmr.l2_normalize(x.contiguous().to(f32), float(eps))[0]
    return L2NormalizeFunction.apply(x, eps)


def adamw_(params, grads, exp_avg, exp_avg_sq, *, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, step=1,
           grad_scale=1.0, step_device=None):
    """``step_device`` (int32 device tensor = completed steps): the step count is read on the device (``step`` ignored)."""
    if step_device is not None:
        N.check(
            N.load().xfmr_adamw_dev(N.ptr(params), N.ptr(grads), N.ptr(exp_avg), N.ptr(exp_avg_sq), params.numel(), lr,
                                    beta1, beta2, eps, weight_decay, N.ptr(step_device), 1, grad_scale, N.stream()),
            "xfmr_adamw_dev",
        )
        return
    N.check(
        N.load().xfmr_adamw(N.ptr(params), N.ptr(grads), N.ptr(exp_avg), N.ptr(exp_avg_sq), params.numel(), lr, beta1,
                            beta2, eps, weight_decay, step, grad_scale, N.stream()),
        "xfmr_adamw",
    )


def step_advance_(step_device):
    N.check(N.load().xfmr_step_advance(N.ptr(step_device), N.stream()), "xfmr_step_advance")


# ---- the optimizer step's options on the device (include/xfmr_hip.h K18b): clip, gradient scale, lr schedule
def _schedule_ids(schedule) -> tuple[int, int, int]:
    """``{"name", "warmup_steps", "total_steps"}`` (or None = constant) -> (XFMR_SCHED_*, W, T)."""
    if schedule is None:
        return N.SCHEDULES["constant"], 0, 0
    unknown = set(schedule) - {"name", "warmup_steps", "total_steps"}
    if unknown:
        raise ValueError(f"schedule: unknown keys {sorted(unknown)}")
    name = schedule.get("name", "constant")
    if name not in N.SCHEDULES:
        raise ValueError(f"schedule name must be one of {sorted(N.SCHEDULES)}; got {name!r}")
    W, T = int(schedule.get("warmup_steps") or 0), int(schedule.get("total_steps") or 0)
    if W < 0 or T < 0:
        raise ValueError(f"schedule: warmup_steps / total_steps must be >= 0, got {W}, {T}")
    if name in ("warmup_linear", "warmup_cosine") and "total_steps" not in schedule:
        raise ValueError(f"schedule {name!r} needs total_steps")
    return N.SCHEDULES[name], W, T


def lr_lambda(schedule, completed_steps: int) -> float:
    """The schedule's factor after ``completed_steps`` optimizer steps: the library's host form of what its kernel
    evaluates (fp64 arithmetic, rounded once to fp32)."""
    sched, W, T = _schedule_ids(schedule)
    return float(N.load().xfmr_lr_lambda(sched, W, T, int(completed_steps)))


def make_opt_cfg(*, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, grad_scale=1.0, clip_mode=None,
                 clip_val=None, schedule=None, step=1, step_device=None) -> N.OptCfg:
    """xfmr_opt_cfg. ``step_device`` (int32 device tensor = completed steps): the step is read on the device (``step``
    ignored), as in :func:`adamw_`. The caller keeps ``step_device`` alive while the record is in use."""
    if clip_mode not in N.CLIP_MODES:
        raise ValueError(f"clip_mode must be one of 'norm', 'value' or None; got {clip_mode!r}")
    mode = N.CLIP_MODES[clip_mode]
    if mode != N.CLIP_NONE and not (clip_val is not None and float(clip_val) > 0.0):
        raise ValueError(f"clip_mode={clip_mode!r} needs clip_val > 0, got {clip_val!r}")
    sched, W, T = _schedule_ids(schedule)
    return N.OptCfg(lr=lr, beta1=beta1, beta2=beta2, eps=eps, weight_decay=weight_decay, grad_scale=grad_scale,
                    clip_mode=mode, clip_val=float(clip_val) if mode != N.CLIP_NONE else 0.0, sched=sched, step_offset=1,
                    warmup_steps=W, total_steps=T, step=int(step), step_device=N.ptr(step_device))


def opt_buffers(grads: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """(ctl, workspace) for a gradient buffer of this size: the 32-byte xfmr_opt_ctl record as 8 fp32 words (N.CTL names
    them) and the first launch's per-workgroup records."""
    ctl = torch.zeros(8, dtype=f32, device=grads.device)
    return ctl, _bytes(N.load().xfmr_opt_workspace(grads.numel()), grads)


def opt_prepare_(cfg: N.OptCfg, grads, workspace, ctl):
    """grads -> ctl (norm, max |g|, clip coefficient, learning rate, non-finite count); two launches, no atomics."""
    if workspace.numel() < N.load().xfmr_opt_workspace(grads.numel()) or ctl.numel() * ctl.element_size() < 32:
        raise ValueError("opt_prepare_: workspace / ctl too small for this gradient buffer (ops.opt_buffers)")
    N.check(N.load().xfmr_opt_prepare(C.byref(cfg), N.ptr(grads), grads.numel(), N.ptr(workspace), N.ptr(ctl), N.stream()),
            "xfmr_opt_prepare")
    return ctl


def adamw_ctl_(cfg: N.OptCfg, params, grads, exp_avg, exp_avg_sq, ctl):
    """The update of :func:`adamw_` with the gradient clipped as ``ctl`` says and the learning rate read from it."""
    if not (params.numel() == grads.numel() == exp_avg.numel() == exp_avg_sq.numel()):
        raise ValueError("adamw_ctl_: params, grads and the moments must have the same number of elements")
    N.check(N.load().xfmr_adamw_ctl(C.byref(cfg), N.ptr(params), N.ptr(grads), N.ptr(exp_avg), N.ptr(exp_avg_sq),
                                    params.numel(), N.ptr(ctl), N.stream()), "xfmr_adamw_ctl")


def grad_accumulate_(acc, grads, first: bool):
    """acc = grads if first else acc + grads."""
    if acc.numel() != grads.numel():
        raise ValueError("grad_accumulate_: acc and grads must have the same number of elements")
    N.check(N.load().xfmr_grad_accumulate(N.ptr(acc), N.ptr(grads), acc.numel(), 1 if first else 0, N.stream()),
            "xfmr_grad_accumulate")
    return acc


@dataclasses.dataclass(frozen=True)
class LossOpts:
    """The options of a loss call that reach ``xfmr_loss_cfg``, with their one set of defaults. What belongs to a single call
    -- ``table_bf16``, ``workspace``, ``prepared``, ``d_tok_zeroed``, the profile events -- is an argument of that call.
    Reads like the dict it replaces: ``opts["mode"]``, ``opts == {...}``."""

    train_head: str | int               # a name of N.LOSS_IDS, or its id
    all_heads: bool | int = True        # False: the train head alone; True: every head; 2: every head but the train head
    mask_false_negatives: bool = True
    mode: int = N.NEG_SHARED
    scale: float = 1.0
    margin: float = 0.5
    precision: str | int = "bf16"
    num_hard_negatives: int = 0
    padded_positions: int = 0           # packed rows: the padded batch's B * L, the densities' denominator (0: the rows given)
    nsplit: int = 0                     # column splits of the launch plan forced by the caller (0: the library's plan;
    nsplit_grad: int = 0                # parity tests walk several plans)

    @classmethod
    def of(cls, opts=None, /, **kw) -> "LossOpts":
        """A record as it is (``kw`` replacing fields), or the record of a dict and / or keywords."""
        if isinstance(opts, cls):
            return opts.replace(**kw) if kw else opts
        return cls(**(dict(opts or {}) | kw))

    def replace(self, **kw) -> "LossOpts":
        """``dataclasses.replace`` without its walk over the fields (4 us a call; the overlapped step makes four variants)."""
        if kw.keys() - self.__dict__.keys():
            raise TypeError(f"LossOpts has no field {sorted(kw.keys() - self.__dict__.keys())}")
        new = object.__new__(LossOpts)
        new.__dict__.update(self.__dict__, **kw)
        return new

    def __getitem__(self, field: str):
        return getattr(self, field)

    def __eq__(self, other):
        if isinstance(other, dict):  # a dict equals the record it would make
            try:
                other = LossOpts(**other)
            except TypeError:
                return False
        return isinstance(other, LossOpts) and dataclasses.astuple(self) == dataclasses.astuple(other)

    @property
    def head_id(self) -> int:
        head = self.train_head
        return N.LOSS_IDS[head] if isinstance(head, str) else int(head)

    def cfg(self, *, flags: int = 0, profile_grad=None, profile_log=None) -> N.LossCfg:
        """xfmr_loss_cfg: ``flags`` OR-ed with XFMR_LOSS_NSPLIT(nsplit) | XFMR_LOSS_NSPLIT_GRAD(nsplit_grad);
        ``profile_grad`` / ``profile_log``: (start, stop) hipEvent_t handles recorded around the gradient-pass / the
        values-only logging-pass kernel (measurement)."""
        assert 0 <= self.nsplit < 256 and 0 <= self.nsplit_grad < 256
        cfg = N.LossCfg(
            train_head=self.head_id, all_heads=int(self.all_heads), mask_false_negatives=int(self.mask_false_negatives),
            mode=self.mode, precision=N.precision_id(self.precision), scale=float(self.scale), margin=float(self.margin),
            num_hard_negatives=int(self.num_hard_negatives), flags=int(flags) | (self.nsplit << 8) | (self.nsplit_grad << 16),
            padded_positions=int(self.padded_positions),
        )
        if profile_grad is not None:
            cfg.profile_grad[0], cfg.profile_grad[1] = profile_grad
        if profile_log is not None:
            cfg.profile_log[0], cfg.profile_log[1] = profile_log
        return cfg

    def op_scalars(self) -> tuple:
        """The eight scalars torch.ops.xfmr.sampled_loss / sampled_loss_lists take, in the schema's (= the fields') order."""
        return (self.head_id, int(self.all_heads), bool(self.mask_false_negatives), int(self.mode), float(self.scale),
                float(self.margin), str(self.precision), int(self.num_hard_negatives))


def _entry_opts(opts, kw: dict, all_heads: bool) -> LossOpts:
    """The options of a public loss entry: the record it was given, or its keywords over the entry's own ``all_heads``
    default (every head for the (B*L) entries, the train head alone for the list and the dense form). A keyword that is no
    field of the record is a TypeError."""
    return LossOpts.of(opts, **kw) if opts is not None else LossOpts(**({"all_heads": all_heads} | kw))


def sampled_loss_workspace(like, T, H, n_rows, opts=None, *, table_bf16=None, **kw):
    """An (unprepared) workspace for sampled_loss(..., workspace=...) on `like`'s device. ``opts`` / ``**kw``: a
    :class:`LossOpts` or its fields by keyword. The size depends on T, H, n_rows, on ``nsplit`` and on whether
    ``num_hard_negatives`` > 0 (csrc/loss.hip: loss_carve); the library is handed the cfg the call will run with.
    ``table_bf16`` is taken so that the keywords of that call can be passed here as they are; the size does not depend on
    it. Any other keyword that is no field of the record is a TypeError."""
    cfg = _entry_opts(opts, kw, True).cfg()
    return _bytes(N.load().xfmr_sampled_loss_workspace_cfg(C.byref(cfg), T, H, n_rows), like)


def sampled_loss_prepare(ws, key_mask, pos_idx, neg_idx, rnorm, n_rows, H, opts=None, *, table_bf16=None, **kw):
    """The index-only half of the loss (query compaction, multiplicities, distinct negatives) into `ws`, on the
    current stream: needs the key mask, not the token embeddings. Follow with sampled_loss(..., workspace=ws,
    prepared=True) with the same options. The pass depends on ``mode`` (shared negatives are histogrammed) and, through the
    workspace's carve, on ``nsplit`` and ``num_hard_negatives`` > 0. ``padded_positions`` is read by neither this pass nor
    the size query -- only by the final reduction of the loss call (run_loss) -- so all three are handed the same cfg.
    ``table_bf16``: as in :func:`sampled_loss_workspace` (the pass reads indices and inverse norms, not the table)."""
    cfg = _entry_opts(opts, kw, True).cfg()
    N.check(
        N.load().xfmr_sampled_loss_prepare(C.byref(cfg), N.ptr(key_mask), N.ptr(pos_idx), N.ptr(neg_idx), N.ptr(rnorm),
                                           n_rows, key_mask.numel(), H, N.ptr(ws), ws.numel(), N.stream()),
        "xfmr_sampled_loss_prepare",
    )


def sampled_loss(tok, key_mask, pos_idx, neg_idx, table, rnorm, opts=None, *, need_grad=True, table_bf16=None,
                 workspace=None, prepared=False, d_tok_zeroed=None, stats_elsewhere=False, profile_grad=None,
                 profile_log=None, **kw):
    """Returns (losses[7], stats[16], d_tok or None). tok: (T,H) or (B,L,H). ``opts`` / ``**kw``: a :class:`LossOpts` or
    its fields by keyword. `workspace` (sampled_loss_workspace) + `prepared=True`: sampled_loss_prepare already ran on it;
    `d_tok_zeroed`: a zero-filled buffer like tok to take the gradient (the call then skips its own memset);
    `stats_elsewhere`: the caller does not read this call's `stats` (XFMR_LOSS_STATS_ELSEWHERE: an InfoNCE gradient pass
    then keeps no count of its negatives; the count-derived entries of `stats` are 0, `losses` and `d_tok` unchanged);
    `profile_grad` / `profile_log`: as in :meth:`LossOpts.cfg`."""
    o = _entry_opts(opts, kw, True)
    H = tok.shape[-1]
    T = tok.numel() // H
    lib = N.load()
    d_tok = (d_tok_zeroed if d_tok_zeroed is not None else torch.empty_like(tok)) if need_grad else None
    flags = 0
    if d_tok_zeroed is not None and need_grad:
        assert d_tok.shape == tok.shape and d_tok.dtype == tok.dtype
        flags = N.LOSS_DTOK_ZEROED
    if stats_elsewhere:
        flags |= N.LOSS_STATS_ELSEWHERE
    cfg = o.cfg(flags=flags, profile_grad=profile_grad, profile_log=profile_log)
    n_rows = table.shape[0]
    losses = _empty((2 * N.NUM_LOSSES,), tok)
    stats = _empty((N.NUM_STATS,), tok)
    if workspace is None:
        assert not prepared
        nbytes = lib.xfmr_sampled_loss_workspace_cfg(C.byref(cfg), T, H, n_rows)
        ws = _bytes(nbytes, tok)
    else:
        ws, nbytes = workspace, workspace.numel()
    fn = lib.xfmr_sampled_loss_prepared if prepared else lib.xfmr_sampled_loss
    N.check(
        fn(C.byref(cfg), N.ptr(tok), N.ptr(key_mask), N.ptr(pos_idx), N.ptr(neg_idx), N.ptr(table), N.ptr(rnorm),
           N.ptr(table_bf16), n_rows, T, H, N.ptr(losses), N.ptr(stats), N.ptr(d_tok), N.ptr(ws), nbytes, N.stream()),
        "xfmr_sampled_loss_prepared" if prepared else "xfmr_sampled_loss",
    )
    return losses, stats, d_tok


def dense_loss(query, cand, target=None, opts=None, *, target_position="first", need_grad=True, need_cand_grad=False, **kw):
    """``EmbedLoss.forward`` on a dense (N,C,H) candidate tensor (``losses.py:128-155``):
    returns (losses[14], stats[16], d_query or None[, d_cand when ``need_cand_grad``])."""
    out = dense_loss_mode(query, cand, target, N.TARGET_MODES[target_position], _entry_opts(opts, kw, False),
                          need_grad=need_grad, need_cand_grad=need_cand_grad)
    return out if need_cand_grad else out[:3]


def dense_loss_mode(query, cand, target, target_mode: int, opts: LossOpts, *, need_grad=True, need_cand_grad=False):
    """:func:`dense_loss` by XFMR_TARGET_* id: always (losses, stats, d_query or None, d_cand or None). The dense kernel is
    fp32 on the candidates it is given: of ``opts`` it reads the heads, ``mask_false_negatives``, ``scale``, ``margin`` and
    ``num_hard_negatives``; ``mode``, ``precision``, ``padded_positions`` and the launch-plan overrides do not apply to it."""
    Nq, H = query.shape
    Cn = cand.shape[1]
    lib = N.load()
    cfg = opts.replace(mode=N.NEG_SHARED, precision="fp32", padded_positions=0, nsplit=0, nsplit_grad=0).cfg()
    losses, stats = _empty((2 * N.NUM_LOSSES,), query), _empty((N.NUM_STATS,), query)
    d_q = torch.empty_like(query) if need_grad else None
    nbytes = lib.xfmr_dense_loss_workspace(Nq, Cn, H)
    ws = _bytes(nbytes, query)
    d_c = torch.empty_like(cand) if need_cand_grad else None
    N.check(
        lib.xfmr_dense_loss_grads(C.byref(cfg), N.ptr(query), N.ptr(cand), N.ptr(target), int(target_mode), Nq, Cn, H,
                                  N.ptr(losses), N.ptr(stats), N.ptr(d_q), N.ptr(d_c), N.ptr(ws), nbytes, N.stream()),
        "xfmr_dense_loss_grads",
    )
    return losses, stats, d_q, d_c


def sampled_loss_lists(query, pos_items, neg_items, table, rnorm, opts=None, *, need_grad=True, table_bf16=None, **kw):
    """List form (compacted queries): returns (losses[7], stats[16], d_query or None). ``opts`` / ``**kw``: a
    :class:`LossOpts` or its fields by keyword."""
    Np, H = query.shape
    Nn = 0 if neg_items is None else neg_items.numel()
    lib = N.load()
    cfg = _entry_opts(opts, kw, False).cfg()
    n_rows = table.shape[0]
    losses, stats = _empty((2 * N.NUM_LOSSES,), query), _empty((N.NUM_STATS,), query)
    d_q = torch.empty_like(query) if need_grad else None
    nbytes = lib.xfmr_sampled_loss_lists_workspace_cfg(C.byref(cfg), Np, Nn, H, n_rows)
    ws = _bytes(nbytes, query)
    N.check(
        lib.xfmr_sampled_loss_lists(C.byref(cfg), N.ptr(query), N.ptr(pos_items), N.ptr(neg_items), Np, Nn,
                                    N.ptr(table), N.ptr(rnorm), N.ptr(table_bf16), n_rows, H, N.ptr(losses),
                                    N.ptr(stats), N.ptr(d_q),
                                    N.ptr(ws), nbytes, N.stream()),
        "xfmr_sampled_loss_lists",
    )
    return losses, stats, d_q


# ------------------------------------------------------------------------------------------------ encoder
def _env_on(name: str) -> bool:
    v = os.environ.get(name, "")
    return bool(v) and v != "0"


def encoder_flags_from_env() -> int:
    """A/B switches -> xfmr_encoder_cfg.flags bits. Read when the cfg of a step is made, so the
    forward and the backward of that step (which share the cfg) agree whatever happens to the environment in between."""
    f = 0
    if _env_on("XFMR_LN_UNFUSED"):
        f |= N.ENC_LN_UNFUSED
    if _env_on("XFMR_FFN_UNFUSED"):
        f |= N.ENC_FFN_UNFUSED
    if _env_on("XFMR_FFN_BWD_UNFUSED"):
        f |= N.ENC_FFN_BWD_UNFUSED
    if os.environ.get("XFMR_DW_SIDE", "") == "0":
        f |= N.ENC_DW_INLINE
    if os.environ.get("XFMR_DW_SIDE", "") == "any":  # (experiments: the side stream below its token threshold too)
        f |= N.ENC_DW_SIDE_ANY
    if os.environ.get("XFMR_DW_PAIR", "") == "0":
        f |= N.ENC_DW_UNPAIRED
    if _env_on("XFMR_REDUCE_HALF_EARLY"):
        f |= N.ENC_REDUCE_HALF_EARLY
    return f


N_HANDLES = 7  # embed_event, context, grads_half_event, profile_kernel, profile_layer, profile_event0, profile_event1
_U64 = (1 << 64) - 1


def encoder_op_args(*, heads, inter, layers, max_pos, precision, ln_eps=1e-12, hidden_dropout=0.0, attn_dropout=0.0,
                    seed=0, causal=True, flags=None, step_device=None, embed_event=None, context=None,
                    grads_half_event=None, extra_flags=0, profile=None, seq_offsets=None, row_pos=None, seq_len=0,
                    batch=0, hidden=0):
    """make_encoder_cfg's keyword arguments -> plain scalars, in plain Python (no ctypes: this runs inside traced code):
    (heads, inter, layers, max_pos, precision, ln_eps, hidden_dropout, attn_dropout, flags, seed, step_device, handles,
    seq_offsets, row_pos, packed_seq_len) -- the arguments of torch.ops.xfmr.encoder behind its three tensors. The rules of
    the cfg live here and nowhere else: ``flags`` None reads the A/B switches of the environment, ``extra_flags`` is
    OR-ed in, ``causal=False`` sets XFMR_ENC_BIDIRECTIONAL; the seed is the signed form of its 64 bits (a schema int);
    ``handles`` = the three event / context handles and the unpacked ``profile``. ``batch`` / ``hidden`` are the tensors'."""
    f = encoder_flags_from_env() if flags is None else int(flags)
    f |= int(extra_flags)
    if not causal:
        f |= N.ENC_BIDIRECTIONAL
    seed = int(seed) & _U64
    if seed >= 1 << 63:
        seed -= 1 << 64
    if not isinstance(precision, str):  # an id: the schema carries the name
        precision = next(k for k, v in N.PRECISIONS.items() if v == int(precision))
    prof = list(profile) if profile else [0, 0, 0, 0]
    handles = [int(embed_event or 0), int(context or 0), int(grads_half_event or 0)] + [int(x or 0) for x in prof]
    return (int(heads), int(inter), int(layers), int(max_pos), precision, float(ln_eps), float(hidden_dropout),
            float(attn_dropout), f, seed, step_device, handles, seq_offsets, row_pos,
            int(seq_len) if seq_offsets is not None else 0)


def encoder_cfg(B, L, H, heads, inter, layers, max_pos, precision, ln_eps, hidden_dropout, attn_dropout, flags, seed,
                step_device, handles, seq_offsets=None, row_pos=None) -> N.EncoderCfg:
    """THE constructor of xfmr_encoder_cfg: the call's shape + :func:`encoder_op_args`'s scalars (all but the last). The
    eager route and the registered ops both build their struct here. ``step_device``: a device tensor or a pointer."""
    h = [int(x) & _U64 for x in handles] + [0] * (N_HANDLES - len(handles))
    if isinstance(step_device, torch.Tensor):
        assert step_device.dtype in (torch.int32, torch.uint32) and step_device.is_cuda
        step_device = step_device.data_ptr()
    return N.EncoderCfg(
        batch=int(B), seq_len=int(L), hidden=int(H), heads=heads, inter=inter, layers=layers, max_pos=max_pos,
        precision=N.precision_id(precision), ln_eps=ln_eps, hidden_dropout=hidden_dropout, attn_dropout=attn_dropout,
        flags=int(flags) & 0xFFFFFFFF, seed=int(seed) & _U64, step_device=step_device or None,
        embed_event=h[0] or None, context=h[1] or None, grads_half_event=h[2] or None,
        profile_kernel=h[3], profile_layer=h[4], profile_events=(C.c_void_p * 2)(h[5] or None, h[6] or None),
        seq_offsets=N.ptr(seq_offsets), row_pos=N.ptr(row_pos), packed_rows=0 if row_pos is None else int(row_pos.numel()),
    )


def make_encoder_cfg(*, batch, seq_len, hidden, **kw) -> N.EncoderCfg:
    """xfmr_encoder_cfg of (batch, seq_len, hidden) and :func:`encoder_op_args`'s keywords: ``heads``, ``inter``, ``layers``,
    ``max_pos``, ``precision``; ``ln_eps``, ``hidden_dropout``, ``attn_dropout``, ``seed``, ``causal``, ``flags``,
    ``extra_flags``; ``step_device``: a uint32 device tensor (or pointer) mixed into the dropout stream on the device;
    ``embed_event``: a hipEvent_t handle the forward records once the key mask exists; ``context``: an
    ``xfmr_context`` handle (side stream of the backward's weight-gradient GEMMs); ``profile``: (N.PROF_*, layer,
    event0, event1) -- HIP events recorded around that part of the encoder (measurement); ``seq_offsets`` (batch + 1,
    int32) + ``row_pos`` (packed rows, int32): the PACKED layout (pack_rows) -- the token axis holds only each
    sequence's own rows."""
    return encoder_cfg(batch, seq_len, hidden, *encoder_op_args(**kw)[:-1])


class Context:
    """Owner of one ``xfmr_context`` (the lowest-priority side stream + fork / join events that ``xfmr_encoder_bwd`` runs
    its weight-gradient GEMMs on). Created on the current device; destroyed with the object."""

    def __init__(self, device=None):
        self.handle = None
        h = C.c_void_p()
        with torch.cuda.device(device):
            N.check(N.load().xfmr_context_create(C.byref(h)), "xfmr_context_create")
        self.handle = h.value

    def close(self):
        if self.handle:
            N.load().xfmr_context_destroy(self.handle)
            self.handle = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


def pack_rows(hist, pos, neg, offsets64, rows: int, order=None):
    """The PACKED layout of a collated batch (xfmr_pack_rows): hist / pos / neg (B, L) int64 device tensors (neg may be
    None), offsets64 (B + 1) int64 on the device = the cumulative row lengths, ``rows`` = offsets64[-1] as the HOST knows
    it (the collate padded the rows: it knows their lengths). ``order`` (B,) int64 on the device: packed slot b holds batch row
    order[b] and offsets64 are the cumulative lengths in THAT order (:func:`length_order`: longest first). Returns the packed
    (rows,) index tensors, ``seq_offsets`` (B + 1) int32 and ``row_pos`` (rows,) int32 for make_encoder_cfg."""
    B, L = hist.shape
    dev = hist.device
    out = {k: torch.empty((rows,), dtype=torch.int64, device=dev) for k in ("hist", "pos")}
    out["neg"] = torch.empty((rows,), dtype=torch.int64, device=dev) if neg is not None else None
    out["seq_offsets"] = torch.empty((B + 1,), dtype=torch.int32, device=dev)
    out["row_pos"] = torch.empty((rows,), dtype=torch.int32, device=dev)
    N.check(N.load().xfmr_pack_rows_ordered(N.ptr(hist), N.ptr(pos), N.ptr(neg), N.ptr(offsets64), N.ptr(order), B, L, rows,
                                            N.ptr(out["hist"]), N.ptr(out["pos"]), N.ptr(out["neg"]), N.ptr(out["seq_offsets"]),
                                            N.ptr(out["row_pos"]), N.stream()), "xfmr_pack_rows_ordered")
    return out


def length_order(lengths):
    """(order, offsets) of a batch's row lengths (CPU int64 tensor) for the packed layout: the rows by length, LONGEST first
    (stable), and the cumulative lengths in that order (B + 1). The attention kernels run one workgroup per (sequence, head)
    in slot order; a 200-token sequence that starts last is a 28 us tail on a launch whose balanced time is ~45 (MovieLens-like
    batches of 512, one-stream trace: attention backward 72.6 -> 58.2 us per layer, forward 26.2 -> 20.2; step 1.867 -> 1.853 ms)."""
    lens = torch.as_tensor(lengths, dtype=torch.int64).cpu()
    if os.environ.get("XFMR_PACK_ORDER", "") == "0":  # (A/B runs: the batch's own order)
        order = torch.arange(lens.numel(), dtype=torch.int64)
    else:
        order = torch.argsort(lens, descending=True, stable=True)
    off = torch.zeros(lens.numel() + 1, dtype=torch.int64)
    torch.cumsum(lens[order], 0, out=off[1:])
    return order, off


def _encoder_outputs(cfg: N.EncoderCfg, flat_params, size_entry: str, head_sizes: str):
    """(tok, key_mask, nbytes of ``size_entry``) for a forward of ``cfg``: (B, L, H) + (B, L), or -- packed layout: the
    token axis holds the sequences' own rows only -- (rows, H) + (rows,). A cfg the library does not build is refused."""
    rows = (cfg.packed_rows,) if cfg.packed_rows else (cfg.batch, cfg.seq_len)
    tok = _empty((*rows, cfg.hidden), flat_params)
    key_mask = _empty(rows, flat_params, torch.uint8)
    nbytes = getattr(N.load(), size_entry)(C.byref(cfg))
    if nbytes == 0:
        raise RuntimeError(f"{size_entry}: unsupported encoder configuration "
                           f"(head size must be {head_sizes}, sizes positive, seq_len <= max_pos)")
    return tok, key_mask, nbytes


def encoder_fwd(cfg: N.EncoderCfg, flat_params, item_idx, table):
    tok, key_mask, nbytes = _encoder_outputs(cfg, flat_params, "xfmr_encoder_workspace_bytes", "32")
    acts = _bytes(nbytes, flat_params)
    N.check(
        N.load().xfmr_encoder_fwd(C.byref(cfg), N.ptr(flat_params), N.ptr(item_idx), N.ptr(table), table.shape[0],
                                  N.ptr(tok), N.ptr(key_mask), N.ptr(acts), nbytes, N.stream()),
        "xfmr_encoder_fwd",
    )
    return tok, key_mask, acts


def encoder_infer_fwd(cfg: N.EncoderCfg, flat_params, item_idx, table, workspace=None):
    """xfmr_encoder_infer: (tok, key_mask, workspace) -- the bits of :func:`encoder_fwd` for the same cfg (dropout 0), with
    nothing kept for a backward. ``workspace``: a byte tensor of at least xfmr_encoder_infer_workspace_bytes(cfg) bytes to
    run in (scratch of this call only); None allocates one of exactly that size."""
    tok, key_mask, nbytes = _encoder_outputs(cfg, flat_params, "xfmr_encoder_infer_workspace_bytes", "32 or 64")
    if workspace is None:
        workspace = torch.empty(int(nbytes), dtype=torch.uint8, device=flat_params.device)
    N.check(
        N.load().xfmr_encoder_infer(C.byref(cfg), N.ptr(flat_params), N.ptr(item_idx), N.ptr(table), table.shape[0],
                                    N.ptr(tok), N.ptr(key_mask), N.ptr(workspace), workspace.numel(), N.stream()),
        "xfmr_encoder_infer",
    )
    return tok, key_mask, workspace


# ------------------------------------------------------------------------------------------------ session encoder
# include/xfmr_session.h. Eager only, no torch.library registration: there is no autograd and nothing to trace. The cfg is
# :func:`make_encoder_cfg`'s (batch = n_slots, seq_len = max_pos by convention; neither is read beyond the cfg check).
def session_plan(cfg: N.EncoderCfg) -> dict:
    """xfmr_session_plan: what the attend kernel does for this cfg -- ``chunk`` (keys per online-softmax step of one wave),
    ``lanes_per_key``, ``keys_per_load``, ``kv_bytes`` per element, ``bf16_storage``, ``max_len``. Touches no device; a cfg
    the session entries refuse raises."""
    out = (C.c_int32 * 8)()
    N.check(N.load().xfmr_session_plan(C.byref(cfg), out), "xfmr_session_plan")
    return dict(chunk=out[0], lanes_per_key=out[1], keys_per_load=out[2], kv_bytes=out[3], bf16_storage=bool(out[4]),
                max_len=out[5])


def session_state_bytes(cfg: N.EncoderCfg, n_slots: int) -> int:
    """Bytes of the state buffer for ``n_slots`` sessions (0: the cfg is refused)."""
    return int(N.load().xfmr_session_state_bytes(C.byref(cfg), int(n_slots)))


def session_workspace_bytes(cfg: N.EncoderCfg, max_rows: int) -> int:
    """Bytes of the scratch of one :func:`session_append` call of up to ``max_rows`` rows (0: refused)."""
    return int(N.load().xfmr_session_workspace_bytes(C.byref(cfg), int(max_rows)))


def session_init(cfg: N.EncoderCfg, flat_params, state, n_slots: int) -> None:
    """xfmr_session_init: carve ``state`` (a uint8 device tensor), zero the mask bytes, convert the parameters (bf16
    storage). Every slot is empty afterwards; call it again after the weights change."""
    N.check(N.load().xfmr_session_init(C.byref(cfg), N.ptr(flat_params), N.ptr(state), state.numel(), int(n_slots),
                                       N.stream()), "xfmr_session_init")


def session_append(cfg: N.EncoderCfg, flat_params, state, n_slots: int, item_idx, row_slot, row_pos, table, workspace,
                   *, want_tok: bool = True):
    """xfmr_session_append: row r = item ``item_idx[r]`` (int64) at position ``row_pos[r]`` of slot ``row_slot[r]`` (int32
    device tensors of one length). Returns the rows' last-layer outputs (n_rows, H), or None with ``want_tok=False``. A row
    with a slot or position out of range stores nothing and comes back as a zero row; no (slot, position) pair twice."""
    n = int(item_idx.numel())
    assert item_idx.dtype == torch.int64 and row_slot.dtype == torch.int32 and row_pos.dtype == torch.int32
    assert row_slot.numel() == n and row_pos.numel() == n
    tok = _empty((n, cfg.hidden), flat_params) if want_tok else None
    N.check(N.load().xfmr_session_append(C.byref(cfg), N.ptr(flat_params), N.ptr(state), state.numel(), int(n_slots),
                                         N.ptr(item_idx), N.ptr(row_slot), N.ptr(row_pos), n, N.ptr(table), table.shape[0],
                                         N.ptr(tok), N.ptr(workspace), workspace.numel(), N.stream()),
            "xfmr_session_append")
    return tok


def session_pool(cfg: N.EncoderCfg, state, n_slots: int, slots, lens, mode: str = "mean", *, normalize: bool = False,
                 eps: float = 1e-12):
    """xfmr_session_pool: :func:`pool` (+ :func:`l2_normalize`) over the stored rows [0, lens[i]) of slot slots[i] (int32
    device tensors). Returns (n, H); a length of 0 gives a zero row."""
    n = int(slots.numel())
    assert slots.dtype == torch.int32 and lens.dtype == torch.int32 and lens.numel() == n
    out = torch.empty((n, cfg.hidden), dtype=f32, device=state.device)
    N.check(N.load().xfmr_session_pool(C.byref(cfg), N.ptr(state), state.numel(), int(n_slots), N.ptr(slots), N.ptr(lens),
                                       n, N.POOL_MODES[mode], int(bool(normalize)), float(eps), N.ptr(out), N.stream()),
            "xfmr_session_pool")
    return out


last_encoder_grad_ptr = 0  # device address of the flat gradient buffer the last xfmr_encoder_bwd call wrote


def encoder_bwd(cfg: N.EncoderCfg, flat_params, d_tok, key_mask, acts, grads=None):
    """d_tok is clobbered. Returns the flat gradient buffer."""
    global last_encoder_grad_ptr
    if grads is None:
        grads = torch.empty_like(flat_params)
    last_encoder_grad_ptr = grads.data_ptr()  # (distributed.HalvedAllReduce checks that .grad IS this buffer)
    N.check(
        N.load().xfmr_encoder_bwd(C.byref(cfg), N.ptr(flat_params), N.ptr(grads), N.ptr(d_tok), N.ptr(key_mask),
                                  N.ptr(acts), acts.numel(), N.stream()),
        "xfmr_encoder_bwd",
    )
    return grads


def backward_scratch(d_tok, same):
    """The buffer an encoder backward runs on. Its kernel sequence uses the incoming gradient as scratch, and may do so in
    place only when the producer handed the buffer over by marking it ``_xfmr_consumable`` (the fused (B*L) loss does: its
    saved gradient is dead after its own backward); otherwise it works on a copy. ``same(d, d_tok)``: whether
    ``contiguous()`` returned its argument -- ``data_ptr()`` equality on real tensors, ``is`` where the tensors may be fake
    (a traced backward)."""
    d = d_tok.contiguous()
    if same(d, d_tok) and not getattr(d_tok, "_xfmr_consumable", False):
        d = d.clone()
    return d


class EncoderFunction(torch.autograd.Function):
    """tok, key_mask = encoder(flat_params, item_idx); backward fills the flat gradient."""

    @staticmethod
    def forward(ctx, flat_params, item_idx, table, cfg, keep=None):
        tok, key_mask, acts = encoder_fwd(cfg, flat_params, item_idx, table)
        ctx.cfg = cfg
        ctx.keep = keep  # tensors the cfg points into (packed layout: seq_offsets, row_pos) live until the backward has run
        ctx.save_for_backward(flat_params, key_mask, acts)
        ctx.mark_non_differentiable(key_mask)
        ctx.set_materialize_grads(False)  # no zero-filled gradient for the mask output
        return tok, key_mask

    @staticmethod
    def backward(ctx, d_tok, _d_mask):
        flat_params, key_mask, acts = ctx.saved_tensors
        if d_tok is None:
            return None, None, None, None, None
        d = backward_scratch(d_tok, lambda a, b: a.data_ptr() == b.data_ptr())
        grads = encoder_bwd(ctx.cfg, flat_params, d, key_mask, acts)
        return grads, None, None, None, None


_UNIT_GRADS: dict = {}


def unit_grad(like: torch.Tensor) -> torch.Tensor:
    """THE scalar 1 on `like`'s device, one persistent tensor per device. ``loss.backward(gradient=ops.unit_grad(loss))``
    does what ``loss.backward()`` does without the per-step ones-fill launch, and the fused loss's backward recognises
    the object and skips its `d_tok *= g` launch (two ~5 us launches between the loss and the encoder backward).
    ``RecommenderLightningModule.backward`` -- Lightning's overridable hook -- passes it."""
    key = (like.device.type, like.device.index)
    t = _UNIT_GRADS.get(key)
    if t is None:
        t = _UNIT_GRADS[key] = torch.ones((), dtype=f32, device=like.device)
    return t


unit_grad_hits = 0  # backward calls that recognised the unit gradient (tests)


def _is_unit_grad(g: torch.Tensor) -> bool:
    global unit_grad_hits
    hit = any(g is t for t in _UNIT_GRADS.values())
    unit_grad_hits += int(hit)
    return hit


class LossFunction(torch.autograd.Function):
    """(train_loss, losses[14], stats[16]) = ``run(need, *inputs)``, the node of all three loss forms. Only train_loss
    carries a gradient: the kernels computed it in the same pass as the values, into one buffer per input of ``slots`` that
    requires a gradient (``need``: which of them do; ``run`` returns ``(losses, stats, buffers)`` with None where not
    needed), and the backward scales the buffers by the incoming gradient, a device scalar. ``sampled``: the (B*L) form of
    the training step, which alone knows the unit gradient, hands its buffer over to the encoder backward and asks for no
    zero-filled gradients of the logging outputs."""

    @staticmethod
    def forward(ctx, run, head: int, slots: tuple, sampled: bool, *inputs):
        losses, stats, grads = run(tuple(inputs[i].requires_grad for i in slots), *inputs)
        ctx.slots = tuple(4 + i for i, d in zip(slots, grads) if d is not None)  # positions among forward's arguments
        ctx.n_in, ctx.sampled = 4 + len(inputs), sampled
        ctx.save_for_backward(*(d for d in grads if d is not None))
        ctx.mark_non_differentiable(losses, stats)
        if sampled:
            ctx.set_materialize_grads(False)
        return losses[head].clone(), losses, stats

    @staticmethod
    def backward(ctx, g, _gl, _gs):
        out = [None] * ctx.n_in
        if g is None:  # (the sampled form alone can see None: the others get a zero-filled gradient)
            return tuple(out)
        saved = ctx.saved_tensors
        if not (ctx.sampled and _is_unit_grad(g)):  # (the persistent unit gradient: nothing to multiply by)
            g = g.contiguous().to(f32)
            for d in saved:
                N.check(N.load().xfmr_scale_by_device_scalar(N.ptr(d), d.numel(), N.ptr(g), N.stream()),
                        "xfmr_scale_by_device_scalar")
        for slot, d in zip(ctx.slots, saved):
            if ctx.sampled and not torch.is_grad_enabled():  # not under create_graph: the buffer is dead after this backward
                d._xfmr_consumable = True
            out[slot] = d
        return tuple(out)


# ------------------------------------------------------------------------------------------------ torch.ops.xfmr.*
# The same implementations registered as PyTorch custom operators (custom_ops.py: schema + fake tensors + autograd
# formulas), so that torch.compile / torch.export of a model built from these kernels sees shape-inferable opaque ops.
# The eager step keeps the autograd.Function route above -- a Python-registered op with an autograd formula costs
# ~130 us of host time per call against ~12 (custom_ops.py) --; traced code, or XFMR_TORCH_OPS=1, takes the ops.
from . import custom_ops  # noqa: E402  (registers torch.ops.xfmr.*)


def use_torch_ops() -> bool:
    return torch.compiler.is_compiling() or os.environ.get("XFMR_TORCH_OPS", "") == "1"


def encoder(flat_params, item_idx, table, cfg_kwargs: dict):
    """tok (B,L,H), key_mask (B,L) = the encoder of `cfg_kwargs` (make_encoder_cfg's keyword arguments) on `item_idx`;
    differentiable in `flat_params`. Eager: EncoderFunction; traced / XFMR_TORCH_OPS=1: torch.ops.xfmr.encoder."""
    if use_torch_ops():
        tok, key_mask, _acts = torch.ops.xfmr.encoder(flat_params, item_idx, table, *encoder_op_args(**cfg_kwargs))
        return tok, key_mask
    keep = (cfg_kwargs.get("seq_offsets"), cfg_kwargs.get("row_pos"))
    return EncoderFunction.apply(flat_params, item_idx, table, make_encoder_cfg(**cfg_kwargs), keep)


def infer_enabled() -> bool:
    """Whether the evaluation surfaces (``encode_batch``, ``encode``, ``DeviceEvalSet.encode`` and what goes through them)
    take the forward-only entry. ``XFMR_INFER=0``, read per call, routes them through the training forward again (A/B
    timing, bisecting): the results are the same bits either way."""
    return os.environ.get("XFMR_INFER", "") != "0"


last_infer_workspace_nbytes = 0  # size of the workspace tensor the last eager encoder_infer call ran in (tests)


def encoder_infer(flat_params, item_idx, table, cfg_kwargs: dict):
    """tok, key_mask of :func:`encoder` for the same ``cfg_kwargs`` (dropout 0), bit for bit, through the forward-only pass
    (xfmr_encoder_infer): nothing is stored for a backward, the workspace is one byte tensor of exactly the library's size
    that dies with the call. No autograd node: the outputs never require grad, and a call that would be expected to
    deliver a gradient -- grad mode on and ``flat_params.requires_grad`` -- raises; use it under ``torch.no_grad()`` /
    ``torch.inference_mode()``. Eager: the C ABI call; traced / XFMR_TORCH_OPS=1: torch.ops.xfmr.encoder_infer."""
    global last_infer_workspace_nbytes
    if torch.is_grad_enabled() and flat_params.requires_grad:
        raise RuntimeError("ops.encoder_infer is forward-only and has no backward: call it under torch.no_grad() / "
                           "torch.inference_mode(), or use ops.encoder for a differentiable forward")
    if use_torch_ops():
        return torch.ops.xfmr.encoder_infer(flat_params, item_idx, table, *encoder_op_args(**cfg_kwargs))
    tok, key_mask, ws = encoder_infer_fwd(make_encoder_cfg(**cfg_kwargs), flat_params.detach(), item_idx, table)
    last_infer_workspace_nbytes = ws.nbytes
    return tok, key_mask


def _grad_on(t) -> bool:
    return bool(t.requires_grad and torch.is_grad_enabled())


def sampled_loss_train(tok, key_mask, pos_idx, neg_idx, table, rnorm, opts, *, table_bf16=None, **eager_only):
    """(train_loss, losses[14], stats[16]) on (B*L) positions; train_loss carries the gradient w.r.t. `tok`. ``opts``: a
    :class:`LossOpts` (or its dict). ``eager_only``: sampled_loss's ``workspace``, ``prepared``, ``d_tok_zeroed``,
    ``stats_elsewhere``, ``profile_grad``, ``profile_log`` -- a call that sets one of them takes the eager route whatever use_torch_ops() says
    (an autograd-registered op must be functional)."""
    o = LossOpts.of(opts)
    if use_torch_ops() and all(v is None or v is False for v in eager_only.values()):
        out = torch.ops.xfmr.sampled_loss(tok, key_mask, pos_idx, neg_idx, table, rnorm, table_bf16, *o.op_scalars(),
                                          _grad_on(tok), [int(o.nsplit), int(o.nsplit_grad)])
        return out[0], out[1], out[2]

    def run(need, *tensors):
        losses, stats, d_tok = sampled_loss(*tensors, o, need_grad=need[0], table_bf16=table_bf16, **eager_only)
        return losses, stats, (d_tok,)

    return LossFunction.apply(run, o.head_id, (0,), True, tok, key_mask, pos_idx, neg_idx, table, rnorm)


def sampled_loss_lists_train(query, pos_items, neg_items, table, rnorm, opts, *, table_bf16=None):
    """List form of :func:`sampled_loss_train`: compacted queries, explicit item-id lists."""
    o = LossOpts.of(opts)
    if use_torch_ops():
        out = torch.ops.xfmr.sampled_loss_lists(query, pos_items, neg_items, table, rnorm, table_bf16, *o.op_scalars(),
                                                _grad_on(query))
        return out[0], out[1], out[2]

    def run(need, *tensors):
        losses, stats, d_q = sampled_loss_lists(*tensors, o, need_grad=need[0], table_bf16=table_bf16)
        return losses, stats, (d_q,)

    return LossFunction.apply(run, o.head_id, (0,), False, query, pos_items, neg_items, table, rnorm)


def dense_loss_train(query, cand, target, opts, *, target_position="first"):
    """``EmbedLoss.forward`` on dense candidates, differentiable in the query and -- when they require a gradient -- in
    the candidates (``losses.py:128-155``)."""
    o, mode = LossOpts.of(opts), N.TARGET_MODES[target_position]
    if use_torch_ops():
        s = o.op_scalars()  # (the dense op's schema: no mode, no precision)
        out = torch.ops.xfmr.dense_loss(query, cand, target, mode, s[0], s[1], s[2], s[4], s[5], s[7], _grad_on(query),
                                        _grad_on(cand))
        return out[0], out[1], out[2]

    def run(need, *tensors):
        losses, stats, d_q, d_c = dense_loss_mode(*tensors, mode, o, need_grad=any(need), need_cand_grad=need[1])
        return losses, stats, (d_q if need[0] else None, d_c)

    return LossFunction.apply(run, o.head_id, (0, 1), False, query, cand, target)
