"""One case per reachable family and tile of the GEMM plan (csrc/gemm_plan.inc: gemm_plan; tests/test_gemm_plan_host.py has the
rules): the library is asked which form a call takes (xf_gemm_plan, with the switches as the library reads them and the
device's compute units), the expected form is asserted, and the same call then runs through the existing entry point over
outputs pre-filled with NaN and is compared with an fp64 reference at the existing tests' tolerances -- so "the plan names form
X" and "form X ran and is right" are asserted together. Smallest shapes at which each form can go wrong: a partial last M-tile
(70 rows) and, where there are several, a partial N-tile; a last slab with a short token chunk; one token past a slab.
Operands of the bf16-storage entries are bf16-representable, so that only the fp32 accumulation remains (helpers.TOL["fp32"])."""

import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import dropout_model as dm
from fused_refs import dx_lnbwd_ref, ffn_bwd_dx_ref
from helpers import assert_close
from test_gemm_plan_host import (AB, BF16, DW, DW_DEFERRED, DW_GROUP, DX, DX_GELU, DX_LNBWD, EPI_DROP_RES_LN,
                                 EPI_DROP_RES_LN_RE, EPI_DROP_RES_LN_RED, EPI_DX_LNBWD, EPI_SPLITK, F32, FFN_BWD, FFN_BWD_KERNEL,
                                 FFN_FWD, FFN_FWD_KERNEL, FIELDS, FWD_BIAS, FWD_DROP_RES, FWD_GELU, GROUP, LN_FWD, LN_FWD_RE,
                                 LN_FWD_RE_DROP, OK, RING, RING_LDS, TILE)
from test_gpu_ffn_bwd_reference import _check_ln_stage, _guarded, _lnbwd_inputs, _run_ffn
from test_gpu_ffn_weight_ring import _inputs as _ffn_bwd_inputs
from xfmr_rec_amd._native import DwItem, LnResidual

pytestmark = pytest.mark.gpu
DEV = "cuda"
H = 128
SEED, SITE, SITE_RES = 5, 9, 2
PREC = {BF16: "bf16", F32: "fp32"}


@pytest.fixture(scope="module")
def N():
    from xfmr_rec_amd import _native

    return _native


@pytest.fixture(scope="module")
def lib(N):
    return N.load()


@pytest.fixture(scope="module")
def plan(lib):
    """The plan of a call under the switches the library reads from the environment right now, on this device."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count

    def ask(op, M, N, K, prec=BF16, s16=0, items=1):
        sw, out = (C.c_int32 * 16)(), (C.c_int32 * 24)()
        lib.xf_gemm_switches(sw)
        assert lib.xf_gemm_plan(op, M, N, K, prec, s16, items, cus, sw, out) == OK
        return dict(zip(FIELDS, out))

    return ask


def nan(shape, dtype=torch.float32):
    """All-ones bytes: NaN as fp32 and as bf16."""
    n = torch.empty(shape, dtype=dtype).numel() * torch.empty((), dtype=dtype).element_size()
    return torch.full((n,), 0xFF, dtype=torch.uint8, device=DEV).view(dtype).view(shape)


def rand(*shape, seed, scale=1.0, bf16=False):
    t = torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale
    return t.to(torch.bfloat16).to(DEV) if bf16 else t.to(DEV)


def tile(p):
    return p["family"], p["bm"], p["bn"], p["bk"]


# ------------------------------------------------------------------------------------------------ the tile kernel
def _forward(lib, N, prec, x, w, b, epilogue, res=None):
    M, K, Nn = x.shape[0], x.shape[1], w.shape[0]
    y, aux = nan((M, Nn)), nan((M, Nn)) if epilogue == N.EPI_BIAS_GELU else None
    N.check(lib.xfmr_linear_fwd(N.ptr(x), N.ptr(w), N.ptr(b), N.ptr(y), M, Nn, K, epilogue, N.ptr(res), N.ptr(aux), 0.0, 0, 0,
                                prec, N.stream()), "xfmr_linear_fwd")
    return y, aux


@pytest.mark.parametrize("prec,M,Nn,K,want", [(BF16, 70, 72, 64, (64, 64, 64)), (BF16, 70, 264, 64, (64, 128, 64)),
                                              (BF16, 70, 72, 96, (64, 64, 32)), (F32, 70, 68, 36, (64, 64, 32))],
                         ids=["bf16-64x64x64", "bf16-64x128x64", "bf16-64x64x32", "fp32-64x64x32"])
def test_tile_kernel_forward_epilogues(lib, N, plan, prec, M, Nn, K, want):
    for op in (FWD_BIAS, FWD_GELU, FWD_DROP_RES):
        assert tile(plan(op, M, Nn, K, prec)) == (TILE, *want), op
    x, w, b, r = rand(M, K, seed=1), rand(Nn, K, seed=2, scale=K**-0.5), rand(Nn, seed=3), rand(M, Nn, seed=4)
    ref = (x.double() @ w.double().T + b.double()).cpu()
    name = PREC[prec]
    y, _ = _forward(lib, N, prec, x, w, b, N.EPI_BIAS)
    assert_close("linear.bias", y, ref, name)
    y, pre = _forward(lib, N, prec, x, w, b, N.EPI_BIAS_GELU)
    assert_close("linear.gelu.pre", pre, ref, name)
    assert_close("linear.gelu", y, F.gelu(ref), name)
    y, _ = _forward(lib, N, prec, x, w, b, N.EPI_BIAS_DROP_RES, r)
    assert_close("linear.residual", y, ref + r.double().cpu(), name)


@pytest.mark.parametrize("prec,M,Nn,K,want,want_gelu", [(BF16, 70, 64, 72, (64, 64, 64), (64, 64, 64)),
                                                        (BF16, 70, 64, 264, (64, 128, 64), (64, 64, 64)),  # gelu' stays at 64
                                                        (BF16, 70, 96, 72, (64, 64, 32), (64, 64, 32)),
                                                        (F32, 70, 36, 68, (64, 64, 32), (64, 64, 32))],
                         ids=["bf16-64x64x64", "bf16-64x128x64", "bf16-64x64x32", "fp32-64x64x32"])
def test_tile_kernel_dx(lib, N, plan, prec, M, Nn, K, want, want_gelu):
    """dx[M,K] = dy[M,N] w[N,K]: the tile follows K, the slice depth N."""
    assert tile(plan(DX, M, Nn, K, prec)) == (TILE, *want) and tile(plan(DX_GELU, M, Nn, K, prec)) == (TILE, *want_gelu)
    dy, w, rg, pre = rand(M, Nn, seed=1), rand(Nn, K, seed=2, scale=Nn**-0.5), rand(M, K, seed=4), rand(M, K, seed=5)
    ref = (dy.double() @ w.double()).cpu()
    name = PREC[prec]

    def run(residual_grad=None, gelu_pre=None):
        dx = nan((M, K))
        N.check(lib.xfmr_linear_bwd_dx(N.ptr(dy), N.ptr(w), N.ptr(dx), M, Nn, K, N.ptr(residual_grad), N.ptr(gelu_pre), prec,
                                       N.stream()), "xfmr_linear_bwd_dx")
        return dx

    assert_close("dx", run(), ref, name, "grad")
    assert_close("dx+res", run(residual_grad=rg), ref + rg.double().cpu(), name, "grad")
    pr = pre.double().cpu().requires_grad_(True)
    F.gelu(pr).backward(ref)
    assert_close("dx*gelu'", run(gelu_pre=pre), pr.grad, name, "grad")


# ------------------------------------------------------------------------------------------------ the weight gradients
def _items(lib, T, shapes, seed=0):
    """bf16 operands and NaN-filled slab / bias-row buffers of one XfDwItem per (N, K)."""
    keep, arr = [], (DwItem * len(shapes))()
    for i, (n, k) in enumerate(shapes):
        dy, x = rand(T, n, seed=seed + 2 * i, scale=0.5, bf16=True), rand(T, k, seed=seed + 2 * i + 1, scale=0.5, bf16=True)
        slabs, bpart = nan((lib.xf_linear_bwd_dw_slab_bytes(T, n, k) // 4,)), nan((256 * n,))
        splits = (C.c_int * 1)()
        arr[i] = DwItem(dy.data_ptr(), x.data_ptr(), n, k, slabs.data_ptr(), bpart.data_ptr(), C.addressof(splits))
        keep.append(dict(dy=dy, x=x, N=n, K=k, slabs=slabs, bias=bpart, splits=splits))
    return arr, keep


def _group(lib, N, arr, n, T):
    rc = lib.xf_linear_bwd_dw_group(arr, n, T, BF16, AB, N.stream())
    assert rc == OK, rc
    torch.cuda.synchronize()


def _one_by_one(lib, N, keep, T):
    for t in keep:
        rc = lib.xf_linear_bwd_dw_deferred(N.ptr(t["dy"]), N.ptr(t["x"]), T, t["N"], t["K"], BF16, AB, N.ptr(t["slabs"]),
                                           N.ptr(t["bias"]), t["splits"], N.stream())
        assert rc == OK, rc
    torch.cuda.synchronize()


def _check_slabs(t, T, p):
    """Every slab against its own token chunk in fp64 (the last one's is short), the bias rows likewise; nothing behind."""
    s, kc, n, k = p["splits"], p["k_chunk"], t["N"], t["K"]
    assert t["splits"][0] == s and (s - 1) * kc < T <= s * kc
    slabs, bias = t["slabs"][: s * n * k].view(s, n, k), t["bias"][: s * n].view(s, n)
    assert torch.isnan(t["slabs"][s * n * k:]).all() and torch.isnan(t["bias"][s * n:]).all()
    dy, x = t["dy"].double().cpu(), t["x"].double().cpu()
    for z in range(s):
        rows = slice(z * kc, min(T, (z + 1) * kc))
        assert_close(f"slab {z}", slabs[z], dy[rows].T @ x[rows], "fp32", "grad")
        assert_close(f"bias row {z}", bias[z], dy[rows].sum(0), "fp32", "grad")
    assert_close("dw", slabs.sum(0), dy.T @ x, "fp32", "grad")


@pytest.mark.parametrize("T,n,k,want,splits", [(300, 192, 136, (128, 64, 128), 3), (200, 64, 64, (64, 64, 128), 2)],
                         ids=["128x64", "64x64"])
def test_split_k_dw_on_the_tile_kernel(lib, N, plan, T, n, k, want, splits):
    """Neither feature count is a multiple of 128: the ring refuses. 300 tokens: slabs of 128, 128 and 44."""
    p = plan(DW_DEFERRED, T, n, k, BF16, AB)
    assert tile(p) == (TILE, *want) and (p["splits"], p["k_chunk"], p["epi"]) == (splits, 128, EPI_SPLITK)
    arr, keep = _items(lib, T, [(n, k)])
    _one_by_one(lib, N, keep, T)
    _check_slabs(keep[0], T, p)
    # the immediate form (fp32 storage, both policies): the same plan, reduced
    for prec in (BF16, F32):
        pi = plan(DW, T, n, k, prec)
        assert tile(pi) == (TILE, want[0], want[1], 128 if prec == BF16 else 32) and pi["splits"] == splits
        dy, x = keep[0]["dy"].float(), keep[0]["x"].float()
        dw, nbytes = nan((n, k)), lib.xfmr_linear_bwd_dw_workspace(T, n, k)
        ws = nan((nbytes // 4,))
        N.check(lib.xfmr_linear_bwd_dw(N.ptr(dy), N.ptr(x), N.ptr(dw), T, n, k, prec, N.ptr(ws), nbytes, N.stream()), "dw")
        assert_close("dw", dw, dy.double().T @ x.double(), "fp32", "grad")


@pytest.mark.parametrize("n_items", [2, 4])
def test_grouped_generic_dw_equals_the_one_by_one_launches(lib, N, plan, n_items):
    T, shapes = 300, [(192, 136), (136, 192), (192, 192), (136, 136)][:n_items]
    plans = [plan(DW_GROUP, T, n, k, BF16, AB, items=n_items) for n, k in shapes]
    assert all(tile(p) == (GROUP, 128, 64, 128) and p["splits"] == 3 for p in plans)
    arr, grouped = _items(lib, T, shapes)
    _group(lib, N, arr, n_items, T)
    _, single = _items(lib, T, shapes)
    assert all(tile(plan(DW_DEFERRED, T, n, k, BF16, AB)) == (TILE, 128, 64, 128) for n, k in shapes)
    _one_by_one(lib, N, single, T)
    for g, s, p in zip(grouped, single, plans):
        _check_slabs(g, T, p)
        assert torch.equal(g["slabs"].view(torch.int32), s["slabs"].view(torch.int32))  # bit for bit, the NaN behind included
        assert torch.equal(g["bias"].view(torch.int32), s["bias"].view(torch.int32))


@pytest.mark.parametrize("T", [64, 3073])  # one stage; one token past a slab of XFMR_DWR_TOKENS
def test_ring_dw_alone_and_grouped(lib, N, plan, T):
    shapes = [(128, 128), (384, 128), (128, 128), (384, 128)]
    plans = [plan(DW_GROUP, T, n, k, BF16, AB, items=4) for n, k in shapes]
    for p, (n, k) in zip(plans, shapes):
        assert tile(p) == (RING, 128, 128, 64) and (p["block"], p["lds"]) == (512, RING_LDS)
        alone = plan(DW_DEFERRED, T, n, k, BF16, AB)
        assert tile(alone) == tile(p) and (alone["splits"], alone["k_chunk"]) == (p["splits"], p["k_chunk"])  # the weight alone
    if T == 3073:
        assert all(p["splits"] >= 2 for p in plans)
    arr, grouped = _items(lib, T, shapes)
    _group(lib, N, arr, 4, T)
    _, single = _items(lib, T, shapes)
    _one_by_one(lib, N, single, T)
    for g, s, p in zip(grouped, single, plans):
        _check_slabs(g, T, p)
        assert torch.equal(g["slabs"].view(torch.int32), s["slabs"].view(torch.int32))
        assert torch.equal(g["bias"].view(torch.int32), s["bias"].view(torch.int32))


# ------------------------------------------------------------------------------------------------ the whole-row kernels
def _keep(M, p, site):
    return torch.from_numpy(dm.hidden_keep(SEED, site, M, H, p).astype("float64") * dm.scale(p))


@pytest.mark.parametrize("K", [128, 512])
@pytest.mark.parametrize("res_mode", ["loaded", "rederived", "rederived-dropout"])
def test_whole_row_forward(lib, N, plan, K, res_mode):
    """Linear + bias + dropout + residual + LayerNorm in one kernel, the residual loaded, re-derived from the LayerNorm that
    produced it, or re-derived and dropped out; limits: test_linear_with_layernorm_in_the_epilogue's fp64 restatement."""
    M, p, p_res = 70, 0.1, 0.1 if res_mode == "rederived-dropout" else 0.0
    op, epi = {"loaded": (LN_FWD, EPI_DROP_RES_LN), "rederived": (LN_FWD_RE, EPI_DROP_RES_LN_RE),
               "rederived-dropout": (LN_FWD_RE_DROP, EPI_DROP_RES_LN_RED)}[res_mode]
    pl = plan(op, M, H, K, BF16, AB)
    assert tile(pl) == (TILE, 64, 128, 64) and (pl["epi"], pl["nt_n"], pl["nt_m"], pl["grid"]) == (epi, 1, 2, 8)
    x, w, b = rand(M, K, seed=1, bf16=True), rand(H, K, seed=2, scale=0.05, bf16=True), rand(H, seed=3)
    gamma, beta = 1 + 0.1 * rand(H, seed=4), 0.1 * rand(H, seed=5)
    o = dict(pre=nan((M, H)), y=nan((M, H)), y16=nan((M, H), torch.bfloat16), mean=nan((M,)), rstd=nan((M,)))
    tail = (p, SEED, SITE, N.ptr(gamma), N.ptr(beta), 1e-12, N.ptr(o["y"]), N.ptr(o["y16"]), N.ptr(o["mean"]), N.ptr(o["rstd"]),
            BF16, AB, N.stream())
    if res_mode == "loaded":
        res = rand(M, H, seed=6)
        res64 = res.double().cpu()
        rc = lib.xf_linear_ln_fwd_ex(N.ptr(x), N.ptr(w), N.ptr(b), N.ptr(o["pre"]), M, H, K, N.ptr(res), *tail)
    else:  # the residual = [dropout of] LayerNorm(rp; g0, b0), from what that LayerNorm stored
        rp, g0, b0 = rand(M, H, seed=6), 1 + 0.1 * rand(H, seed=7), 0.1 * rand(H, seed=8)
        mean0 = rp.mean(-1).contiguous()
        rstd0 = (rp.var(-1, unbiased=False) + 1e-12).rsqrt().contiguous()
        res64 = ((rp.double() - mean0.double()[:, None]) * rstd0.double()[:, None] * g0.double() + b0.double()).cpu()
        if p_res > 0:
            res64 = res64 * _keep(M, p_res, SITE_RES)
        r = LnResidual(N.ptr(rp), N.ptr(mean0), N.ptr(rstd0), N.ptr(g0), N.ptr(b0), p_res, SITE_RES)
        rc = lib.xf_linear_ln_fwd_re(N.ptr(x), N.ptr(w), N.ptr(b), N.ptr(o["pre"]), M, H, K, C.byref(r), *tail)
    assert rc == OK, rc
    torch.cuda.synchronize()
    pre64 = _keep(M, p, SITE) * (x.double() @ w.double().T + b.double()).cpu() + res64
    torch.testing.assert_close(o["pre"].double().cpu(), pre64, rtol=2e-5, atol=2e-5)
    ln64 = F.layer_norm(pre64, (H,), gamma.double().cpu(), beta.double().cpu(), 1e-12)
    torch.testing.assert_close(o["y"].double().cpu(), ln64, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(o["mean"].double().cpu(), pre64.mean(-1), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(o["rstd"].double().cpu(), (pre64.var(-1, unbiased=False) + 1e-12).rsqrt(), rtol=1e-5, atol=1e-6)
    assert torch.equal(o["y16"], o["y"].to(torch.bfloat16))


def test_dx_with_layernorm_backward(lib, N, plan):
    M, Nn = 70, 384
    pl = plan(DX_LNBWD, M, Nn, H, BF16, AB)
    assert tile(pl) == (TILE, 64, 128, 64) and (pl["epi"], pl["records"], pl["grid"]) == (EPI_DX_LNBWD, 2, 8)
    t = _lnbwd_inputs(M, Nn)
    n_tiles = lib.xf_ln_row_tiles(M)
    o = dict(dx=_guarded(M, H, torch.float32), parts=_guarded(n_tiles, 3 * H, torch.float32), dlin=_guarded(M, H, torch.bfloat16))
    blocks = C.c_int(0)
    rc = lib.xf_linear_bwd_dx_lnbwd_ex(N.ptr(t["dy"]), N.ptr(t["w"]), M, Nn, H, N.ptr(t["rg"]), N.ptr(t["lnx"]),
                                           N.ptr(t["mean"]), N.ptr(t["rstd"]), N.ptr(t["gamma"]), 0.0, SEED, SITE, N.ptr(o["dx"]),
                                           N.ptr(o["dlin"]), N.ptr(o["parts"]), C.byref(blocks), BF16, AB, N.stream(), 0.0, 0)
    assert rc == OK, rc
    torch.cuda.synchronize()
    assert blocks.value == pl["records"] == n_tiles
    ref = dx_lnbwd_ref(t["dy"], t["w"], t["rg"], t["lnx"], t["gamma"], None, 0.0)
    _check_ln_stage("dx_lnbwd forms", o, ref, M, blocks.value, n_tiles, None, 0.0, True)


@pytest.mark.parametrize("chunk", ["64", "128"])
@pytest.mark.parametrize("I", [128, 256])
def test_fused_ffn_forward(lib, N, plan, monkeypatch, I, chunk):
    """Limits: test_ffn_forward_in_one_kernel_vs_the_two_gemm_form's fp64 restatement of the kernel's own rounding points."""
    M, p = 70, 0.1
    monkeypatch.setenv("XFMR_FFN_CHUNK", chunk)  # read per call, by the plan's switches too
    pl = plan(FFN_FWD, M, H, I)
    assert (pl["family"], pl["ffn_chunk"], pl["epi"], pl["nt_m"], pl["grid"], pl["block"]) == (FFN_FWD_KERNEL, int(chunk),
                                                                                             EPI_DROP_RES_LN, 2, 8, 256)
    x16, w1, b1 = rand(M, H, seed=1, bf16=True), rand(I, H, seed=2, scale=0.08, bf16=True), 0.1 * rand(I, seed=3)
    w2, b2, res = rand(H, I, seed=4, scale=0.05, bf16=True), 0.1 * rand(H, seed=5), rand(M, H, seed=6)
    gamma, beta = 1 + 0.1 * rand(H, seed=7), 0.1 * rand(H, seed=8)
    o = dict(u=nan((M, I), torch.bfloat16), g=nan((M, I), torch.bfloat16), pre=nan((M, H)), y=nan((M, H)),
             y16=nan((M, H), torch.bfloat16), mean=nan((M,)), rstd=nan((M,)))
    rc = lib.xf_ffn_fwd_fused_ex(N.ptr(x16), N.ptr(w1), N.ptr(b1), N.ptr(w2), N.ptr(b2), N.ptr(o["u"]), N.ptr(o["g"]),
                                 N.ptr(o["pre"]), M, H, I, N.ptr(res), p, SEED, SITE, N.ptr(gamma), N.ptr(beta), 1e-12,
                                 N.ptr(o["y"]), N.ptr(o["y16"]), N.ptr(o["mean"]), N.ptr(o["rstd"]), N.stream())
    assert rc == OK, rc
    torch.cuda.synchronize()
    u = (x16.double() @ w1.double().T + b1.double()).to(torch.bfloat16)
    assert int((u != o["u"]).sum()) <= 2e-3 * u.numel()
    gg = F.gelu(u.double()).to(torch.bfloat16)
    assert int((gg != o["g"]).sum()) <= 2e-3 * gg.numel()
    pre = _keep(M, p, SITE) * (o["g"].double() @ w2.double().T + b2.double()).cpu() + res.double().cpu()
    torch.testing.assert_close(o["pre"].double().cpu(), pre, rtol=2e-5, atol=2e-5)
    ln = F.layer_norm(pre, (H,), gamma.double().cpu(), beta.double().cpu(), 1e-12)
    torch.testing.assert_close(o["y"].double().cpu(), ln, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(o["mean"].double().cpu(), pre.mean(-1), rtol=1e-5, atol=1e-5)
    assert torch.equal(o["y16"], o["y"].to(torch.bfloat16))


@pytest.mark.parametrize("staging", ["ring", "registers"])
@pytest.mark.parametrize("I", [64, 192])
def test_fused_ffn_backward(lib, plan, monkeypatch, I, staging):
    """The second stage is judged from the kernel's own dI, as in test_fused_ffn_backward_dx_against_fp64."""
    M = 70
    if staging == "registers":
        monkeypatch.setenv("XFMR_FFN_REG_STAGE", "1")
    else:
        monkeypatch.delenv("XFMR_FFN_REG_STAGE", raising=False)
    pl = plan(FFN_BWD, M, H, I)
    assert (pl["family"], pl["ffn_ring"], pl["records"], pl["grid"], pl["block"]) == (FFN_BWD_KERNEL, int(staging == "ring"), 2, 8, 256)
    t = _ffn_bwd_inputs(M, I)
    o, blocks, n_tiles = _run_ffn(lib, t, M, I, 0.0, True, True)
    assert blocks == pl["records"]
    di = o["di"][:M].cpu()
    want = ffn_bwd_dx_ref(t["dy"], t["w2"], t["u"], t["w1"], None, t["lnx"], t["gamma"], None, 0.0)["di"].to(torch.bfloat16)
    assert bool(((di.double() - want.double()).abs() <= 2.0 ** -7 * want.double().abs() + 1e-6).all())
    assert int((di != want).sum()) <= 2e-3 * di.numel()
    ref = ffn_bwd_dx_ref(t["dy"], t["w2"], t["u"], t["w1"], t["rg"], t["lnx"], t["gamma"], None, 0.0, di=di)
    _check_ln_stage(f"ffn_bwd forms I={I} {staging}", o, ref, M, blocks, n_tiles, None, 0.0, True)
