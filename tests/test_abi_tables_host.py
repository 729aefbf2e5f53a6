"""CPU-side test (no GPU, nothing compiled) of xfmr_rec_amd/_abi.py: the two signature tables and the Structure mirrors are
explicit Python, and this file is what ties them to the C headers. A small parser reads the prototypes and struct bodies of
include/xfmr_hip.h and csrc/internal.h (and XfSeed from csrc/common.h); C types and ctypes types are sorted into the same
classes -- pointer, i32, u32, i64, u64, f32, bool, seed, void -- and compared position by position. (Classes, not
identities: c_size_t is c_uint64 and c_int is c_int32 here.) The comparison is shown to see an argument dropped, an integer
widened, a pointer and a float exchanged and two struct fields exchanged, on in-memory copies."""

import ctypes as C
import pathlib
import re

import pytest

from xfmr_rec_amd import _abi
from xfmr_rec_amd import _native as N

ROOT = pathlib.Path(__file__).resolve().parents[1]
CSRC = ROOT / "transformer-recommenders_amd" / "csrc"
PUBLIC_H, INTERNAL_H, COMMON_H = ROOT / "include" / "xfmr_hip.h", CSRC / "internal.h", CSRC / "common.h"

# ---------------------------------------------------------------------------------------------- the C side
C_SCALARS = {"int32_t": "i32", "int": "i32", "uint32_t": "u32", "unsigned": "u32", "int64_t": "i64", "uint64_t": "u64",
             "size_t": "u64", "float": "f32", "bool": "bool", "XfSeed": "seed", "void": "void"}
C_POINTER_TYPES = {"hipStream_t"}


def clean(text):
    """Without comments, continued lines joined, without preprocessor lines."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = text.replace("\\\n", " ")
    return "\n".join(line for line in text.split("\n") if not line.lstrip().startswith("#"))


def block(text, start):
    """(the text between the brace at or after `start` and its partner, the index behind the partner)."""
    i = text.index("{", start)
    depth = 0
    for j in range(i, len(text)):
        depth += {"{": 1, "}": -1}.get(text[j], 0)
        if depth == 0:
            return text[i + 1:j], j + 1
    return text[i + 1:], len(text)  # the public header closes its extern "C" inside an #ifdef, which clean() removed


def c_class(decl):
    """Class of one parameter or return type: `decl` is the declaration without the parameter's name."""
    if "*" in decl or "[" in decl or "&" in decl:
        return "ptr"
    words = [w for w in decl.split() if w not in ("const", "struct")]
    if len(words) == 1 and words[0] in C_POINTER_TYPES:
        return "ptr"
    return C_SCALARS.get(" ".join(words), "other:" + " ".join(words))


def c_param(text):
    """Class of `type name [= default]`, `type name[n]` or a lone `type`."""
    text = text.split("=")[0].strip()
    m = re.fullmatch(r"(.*?[\s\*&])(\w+)\s*((?:\[\w*\])?)", text, re.S)
    return c_class(text if m is None else m.group(1) + m.group(3))


def prototypes(text, prefix):
    """{name: (return class, [parameter classes])} of every `ret name(args);` whose name starts with the prefix."""
    out = {}
    for m in re.finditer(r"([\w\s\*]+?)\b(" + prefix + r"\w+)\s*\(([^()]*)\)\s*;", text):
        ret, name, args = m.group(1).strip(), m.group(2), m.group(3).strip()
        assert name not in out, f"{name} declared twice"
        out[name] = (c_class(ret), [] if args in ("", "void") else [c_param(a) for a in args.split(",")])
    return out


def structs(text):
    """{name: [(field, class, array length or 0)]} of `typedef struct x {...} x;` and `struct X {...};`. Member functions
    (a declaration with parentheses, its body replaced by a semicolon) are no fields."""
    out = {}
    for m in re.finditer(r"\bstruct\s+(\w+)\s*\{", text):
        body, _ = block(text, m.start())
        while re.search(r"\{[^{}]*\}", body):
            body = re.sub(r"\{[^{}]*\}", ";", body)
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            if "(" in decl:
                continue
            first, *rest = [d.strip() for d in decl.split(",")]
            m2 = re.fullmatch(r"(.*?[\s\*])(\w+)\s*((?:\[\w*\])?)", first, re.S)
            base = m2.group(1)
            for name, arr in [(m2.group(2), m2.group(3))] + [re.fullmatch(r"(\w+)\s*((?:\[\w*\])?)", r).groups() for r in rest]:
                fields.append((name, c_class(base), int(arr[1:-1]) if arr else 0))
        out[m.group(1)] = fields
    return out


def without_structs(text):
    """The text with every struct and enum body cut out: what is left of a header holds its prototypes."""
    while True:
        m = re.search(r"\b(?:struct|enum)\b[^;{()]*\{", text)
        if m is None:
            return text
        _, end = block(text, m.start())
        text = text[:m.start()] + ";" + text[end:]


def extern_c(text):
    """The bodies of all `extern "C" { ... }` blocks, and the one-declaration form `extern "C" ret name(...)`."""
    parts, pos = [], 0
    for m in re.finditer(r'extern\s+"C"\s*', text):
        if m.start() < pos:
            continue
        if text[m.end():m.end() + 1] == "{":
            body, pos = block(text, m.end())
            parts.append(body)
        else:
            parts.append(text[m.end():text.index("\n", m.end())])
    return "\n".join(parts)


PUBLIC_TEXT, INTERNAL_TEXT = clean(PUBLIC_H.read_text()), clean(INTERNAL_H.read_text())
PUBLIC_PROTOS = prototypes(without_structs(PUBLIC_TEXT), "xfmr_")
INTERNAL_PROTOS = prototypes(without_structs(extern_c(INTERNAL_TEXT)), "xf_")
C_STRUCTS = structs(PUBLIC_TEXT) | structs(INTERNAL_TEXT) | structs(clean(COMMON_H.read_text()))
MIRRORS = {"EncoderCfg": "xfmr_encoder_cfg", "LossCfg": "xfmr_loss_cfg", "OptCfg": "xfmr_opt_cfg", "Seed": "XfSeed",
           "DwItem": "XfDwItem", "ReduceSeg": "XfReduceSeg", "LnResidual": "XfLnResidual"}


# ---------------------------------------------------------------------------------------------- the ctypes side
def ct_class(t):
    if t is None:
        return "void"
    if t is _abi.Seed:
        return "seed"
    if t in (C.c_void_p, C.c_char_p) or issubclass(t, (C._Pointer, C.Array)):
        return "ptr"
    if t is C.c_bool:
        return "bool"
    if t is C.c_float:
        return "f32"
    if issubclass(t, C._SimpleCData) and t._type_ in "bhilqBHILQ":
        return ("i" if t._type_.islower() else "u") + str(8 * C.sizeof(t))
    return f"other:{t.__name__}"


def ct_fields(structure):
    return [(name, ct_class(t._type_ if issubclass(t, C.Array) else t), t._length_ if issubclass(t, C.Array) else 0)
            for name, t in structure._fields_]


# ---------------------------------------------------------------------------------------------- the comparison
def table_problems(protos, table, not_bound=()):
    """Every disagreement between a header's prototypes and a table, as text; empty when they agree."""
    bad = [f"{n}: in the header, in no table" for n in sorted(set(protos) - set(table) - set(not_bound))]
    bad += [f"{n}: in the table, not in the header" for n in sorted((set(table) | set(not_bound)) - set(protos))]
    bad += [f"{n}: both bound and listed as not bound" for n in sorted(set(table) & set(not_bound))]
    for name in sorted(set(protos) & set(table)):
        (c_ret, c_args), (res, args) = protos[name], table[name]
        got = [ct_class(a) for a in args]
        if ct_class(res) != c_ret:
            bad.append(f"{name}: returns {c_ret}, the table says {ct_class(res)}")
        if len(got) != len(c_args):
            bad.append(f"{name}: {len(c_args)} parameters, the table has {len(got)}")
        bad += [f"{name}: parameter {i} is {c}, the table says {g}" for i, (c, g) in enumerate(zip(c_args, got)) if c != g]
        bad += [f"{name}: {c} has no class" for c in [c_ret, *c_args, *got] if c.startswith("other")]
    return bad


def struct_problems(structure, c_name):
    want, got = C_STRUCTS[c_name], ct_fields(structure)
    if len(want) != len(got):
        return [f"{c_name}: {len(want)} fields, the mirror has {len(got)}"]
    return [f"{c_name}.{w[0]}: {w}, the mirror has {g}" for w, g in zip(want, got) if w != g]


# ---------------------------------------------------------------------------------------------- the tests
def test_the_parser_reads_every_form_the_headers_use():
    assert len(PUBLIC_PROTOS) == 90 and len(INTERNAL_PROTOS) == 40
    assert PUBLIC_PROTOS["xfmr_abi_version"] == ("i32", [])  # (void)
    assert PUBLIC_PROTOS["xfmr_strerror"] == ("ptr", ["i32"]) and PUBLIC_PROTOS["xfmr_lr_lambda"][0] == "f32"
    assert INTERNAL_PROTOS["xf_gemm_switches"] == ("void", ["ptr"])  # int32_t sw[16]
    assert INTERNAL_PROTOS["xf_dw_ring_takes"][0] == "bool" and INTERNAL_PROTOS["xf_loss_switches"] == ("u64", [])
    assert INTERNAL_PROTOS["xf_attn_fwd_ex"][1][-3:] == ["ptr", "ptr", "bool"]  # hipStream_t, = nullptr, = false
    assert INTERNAL_PROTOS["xf_linear_bwd_dx_lnbwd_ex"][1][-2:] == ["f32", "u32"]  # = 0.f, = 0
    assert INTERNAL_PROTOS["xf_layernorm_bwd_impl"][1].count("other:XfDropout") == 2
    assert "gemm_plan" not in INTERNAL_PROTOS and "gemm_switches" not in INTERNAL_PROTOS  # C++ linkage, no xf_ name
    assert "row_plan" not in INTERNAL_PROTOS and INTERNAL_PROTOS["xf_row_plan"] == ("i32", ["i32", "i64", "i32", "i32", "i32", "ptr"])
    assert ("profile_events", "ptr", 2) in C_STRUCTS["xfmr_encoder_cfg"] and ("pad", "u32", 3) in C_STRUCTS["xfmr_opt_ctl"]
    assert C_STRUCTS["XfDwItem"][2:4] == [("N", "i32", 0), ("K", "i32", 0)]  # int32_t N, K; on a line of several
    assert C_STRUCTS["xfmr_opt_cfg"][:2] == [("lr", "f32", 0), ("beta1", "f32", 0)]
    assert C_STRUCTS["XfSeed"] == [("seed", "u64", 0), ("dyn", "ptr", 0)]  # the constructor is no field
    assert ct_class(C.c_size_t) == "u64" and ct_class(C.c_int) == "i32" and ct_class(C.POINTER(C.c_int32)) == "ptr"
    assert ct_class(C.c_void_p * 2) == "ptr" and ct_class(C.c_double) == "other:c_double"


def test_the_public_table_is_the_public_header():
    assert table_problems(PUBLIC_PROTOS, _abi.SIGNATURES) == []
    assert not [n for n in _abi.SIGNATURES if not n.startswith("xfmr_")]
    assert N.EXPORTED_SYMBOLS == tuple(_abi.SIGNATURES) and N._SIGNATURES is _abi.SIGNATURES


def test_the_internal_table_is_the_internal_header():
    not_bound = dict(_abi.NOT_BOUND)
    assert table_problems(INTERNAL_PROTOS, _abi.INTERNAL_SIGNATURES, not_bound) == []
    assert set(not_bound) == {"xf_layernorm_bwd_impl", "xf_dw_ring_launch_plans"} and all(not_bound.values())
    assert not [n for n in _abi.INTERNAL_SIGNATURES if not n.startswith("xf_") or n.startswith("xfmr_")]
    assert N.INTERNAL_SYMBOLS == tuple(_abi.INTERNAL_SIGNATURES) and not set(N.INTERNAL_SYMBOLS) & set(N.EXPORTED_SYMBOLS)
    # C++ default arguments are rows at full arity
    assert len(_abi.INTERNAL_SIGNATURES["xf_attn_fwd_ex"][1]) == 17 and len(_abi.INTERNAL_SIGNATURES["xf_attn_bwd_ex"][1]) == 19
    assert len(_abi.INTERNAL_SIGNATURES["xf_linear_bwd_dx_lnbwd_ex"][1]) == 22


def test_what_python_calls_is_defined_with_c_linkage_and_declared():
    """The table's names are the internal entries Python calls: each is defined extern "C" in a csrc/*.hip file, and every
    extern "C" xf_* function defined there -- those that Python calls among them -- has its prototype in internal.h."""
    defined = set()
    for src in sorted(CSRC.glob("*.hip")):
        defined |= set(re.findall(r"^[\w\*]+[\s\*]+(xf_\w+)\s*\([^;{}()]*\)\s*\{", extern_c(clean(src.read_text())), re.M))
    called = set(_abi.INTERNAL_SIGNATURES)
    assert len(called) == 38 and called <= defined, sorted(called - defined)
    assert defined <= set(INTERNAL_PROTOS), sorted(defined - set(INTERNAL_PROTOS))


@pytest.mark.parametrize("mirror", sorted(MIRRORS))
def test_structure_mirrors_match_their_c_structs(mirror):
    structure = getattr(_abi, mirror)
    assert struct_problems(structure, MIRRORS[mirror]) == []
    assert getattr(N, mirror) is structure  # what the package and the tests use is the one mirror
    assert not [f for f in ct_fields(structure) if f[1].startswith("other")]


def test_structure_sizes():
    assert C.sizeof(_abi.EncoderCfg) == 136
    assert C.sizeof(_abi.Seed) == 16 and C.sizeof(_abi.ReduceSeg) == 32 and C.sizeof(_abi.DwItem) == 48
    assert C.sizeof(_abi.LnResidual) == 48


def test_bind_types_every_entry_of_the_built_library():
    if not N.LIB_PATH.exists():
        pytest.fail(f"{N.LIB_PATH} missing: run build() first")
    lib = _abi.bind(C.CDLL(str(N.LIB_PATH)))
    for table in (_abi.SIGNATURES, _abi.INTERNAL_SIGNATURES):
        for name, (res, args) in table.items():
            fn = getattr(lib, name)
            assert fn.argtypes == args and fn.restype is res, name
    loaded = N.load()  # load() binds the same tables once: N.load().xf_* is typed everywhere
    assert loaded.xf_ln_row_tiles.argtypes == [C.c_int64] and loaded.xf_dw_ring_takes.restype is C.c_bool
    assert loaded.xf_ln_row_tiles(64 * 5 + 1) >= 6 and loaded.xf_attn_switches() >= 0  # host-only entries, typed

    class Lacking:  # a library without one of the symbols: the error names it
        _name = "lacking.so"

        def __getattr__(self, name):
            if name == "xf_rowsum":
                raise AttributeError(name)
            return getattr(lib, name)

    with pytest.raises(AttributeError, match="lacking.so does not export xf_rowsum"):
        _abi.bind(Lacking())


def test_the_comparison_sees_a_changed_row_and_a_changed_struct():
    """In-memory copies only: no file is touched, nothing is launched."""
    def changed(table, name, edit):
        res, args = table[name]
        copy = dict(table)
        copy[name] = (res, edit(list(args)))
        return copy

    dropped = changed(_abi.INTERNAL_SIGNATURES, "xf_ffn_bwd_dx_fused_ex", lambda a: a[:7] + a[8:])
    got = table_problems(INTERNAL_PROTOS, dropped, dict(_abi.NOT_BOUND))
    assert "xf_ffn_bwd_dx_fused_ex: 21 parameters, the table has 20" in got and all(g.startswith("xf_ffn_bwd_dx_fused_ex") for g in got)

    def widen(a):
        assert a[5] is C.c_int32
        return a[:5] + [C.c_int64] + a[6:]

    got = table_problems(PUBLIC_PROTOS, changed(_abi.SIGNATURES, "xfmr_linear_fwd", widen))
    assert got == ["xfmr_linear_fwd: parameter 5 is i32, the table says i64"]

    def swap(a):
        assert a[7] is C.c_void_p and a[8] is C.c_float  # residual, dropout_p
        return a[:7] + [a[8], a[7]] + a[9:]

    got = table_problems(INTERNAL_PROTOS, changed(_abi.INTERNAL_SIGNATURES, "xf_linear_ln_fwd_ex", swap), dict(_abi.NOT_BOUND))
    assert got == ["xf_linear_ln_fwd_ex: parameter 7 is ptr, the table says f32",
                   "xf_linear_ln_fwd_ex: parameter 8 is f32, the table says ptr"]

    class Exchanged(C.Structure):
        _fields_ = [f if i not in (2, 4) else _abi.DwItem._fields_[6 - i] for i, f in enumerate(_abi.DwItem._fields_)]

    assert [n for n, _ in Exchanged._fields_][2:5] == ["slabs", "K", "N"] and C.sizeof(Exchanged) == C.sizeof(_abi.DwItem)
    got = struct_problems(Exchanged, "XfDwItem")
    assert len(got) == 2 and got[0].startswith("XfDwItem.N:") and got[1].startswith("XfDwItem.slabs:")
    # a return type, a missing row and a stray one are seen too
    other = _abi.SIGNATURES | {"xfmr_lr_lambda": (C.c_int, _abi.SIGNATURES["xfmr_lr_lambda"][1])}
    assert table_problems(PUBLIC_PROTOS, other) == ["xfmr_lr_lambda: returns f32, the table says i32"]
    fewer = {k: v for k, v in _abi.SIGNATURES.items() if k != "xfmr_topk"}
    assert table_problems(PUBLIC_PROTOS, fewer) == ["xfmr_topk: in the header, in no table"]
    assert table_problems(PUBLIC_PROTOS, _abi.SIGNATURES | {"xfmr_nothing": (C.c_int, [])}) == [
        "xfmr_nothing: in the table, not in the header"]


# dir(_native) without underscore names at the commit before the tables moved to _abi.py: bench.py and the package read these
PARENT_NAMES = """ABI_VERSION ATTN_BIDIRECTIONAL ATTN_CAUSAL ATTN_STREAM_KEYS C CLIP_MODES CLIP_NONE CLIP_NORM CLIP_VALUE
COMM_ID_BYTES CTL ECOMM ENC_BIDIRECTIONAL ENC_DW_INLINE ENC_DW_SIDE_ANY ENC_DW_UNPAIRED ENC_FFN_BWD_UNFUSED ENC_FFN_UNFUSED
ENC_LN_UNFUSED ENC_REDUCE_HALF_EARLY EPI_BIAS EPI_BIAS_DROP_RES EPI_BIAS_GELU EXPORTED_SYMBOLS EncoderCfg LIB_PATH
LOSS_DTOK_ZEROED LOSS_IDS LOSS_STATS_ELSEWHERE LossCfg MAX_RANK_CUTOFFS NEG_CATALOG NEG_SHARED NUM_LOSSES NUM_STATS
NativeLibraryError OptCfg POOL_MODES PRECISIONS PREC_BF16 PREC_F32 PROF_ATTN_BWD PROF_ATTN_FWD PROF_DW PROF_FFN_BWD
PROF_FFN_FWD PROF_REDUCE RANK_NONE SCHEDULES STAT Seed TARGET_DIAGONAL TARGET_EXPLICIT TARGET_FIRST TARGET_MODES annotations
check load os pathlib precision_id ptr stream torch""".split()


def test_every_public_name_of_the_parent_still_resolves():
    assert len(PARENT_NAMES) == 64
    assert [n for n in PARENT_NAMES if not hasattr(N, n)] == []
    assert N.Seed.from_param(7).seed == 7 and N.Seed.from_param(7).dyn is None  # a plain int still converts
    assert len(N.EXPORTED_SYMBOLS) == 90 and all(n.startswith("xfmr_") for n in N.EXPORTED_SYMBOLS)


def test_abi_module_needs_nothing_but_ctypes():
    """The plan tests' child processes load it by file path without torch (tests/abi_worker.py): no import but ctypes."""
    src = (ROOT / "transformer-recommenders_amd" / "xfmr_rec_amd" / "_abi.py").read_text()
    imports = re.findall(r"^\s*(?:import|from)\s+([\w\.]+)", src, re.M)
    assert sorted(set(imports)) == ["__future__", "ctypes"]
