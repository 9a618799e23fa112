"""The C-ABI shared library loads without a GPU and exports exactly the entry points include/upnerf_hip.h declares
(no compute calls here); every struct, signature and constant of the ctypes binding agrees with that header (tests/abi_check.py).
Also: the binding refuses to work without the library (no fallback)."""
import ctypes
import os
import subprocess

import pytest

import abi_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "upnerf_hip.h")
# constants of the header that no Python code needs (a new define lands here or in _lib, a mirrored one may not stay here)
UNMIRRORED = ("EINVAL", "EUNSUP", "TILE_ROWS", "MAX_FRAG_DESC", "MAX_PACK_DESC", "VIT_PATCH", "VIT_HEAD_DIM", "BAKED_MAX_SAMPLES")


def test_header_symbols_are_exported_and_bound():
    from upnerf_amd import _lib
    names = sorted(abi_check.prototypes(HEADER))
    assert len(names) >= 15
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(dll, n), f"{n} declared in include/upnerf_hip.h but not exported"
    assert sorted(_lib.EXPORTS) == names, "ctypes binding and header disagree"
    assert _lib.lib.upnerf_abi_version() == _lib.ABI_VERSION == 11


def test_every_struct_mirror_has_the_c_layout():
    """Every ctypes.Structure of _lib against its typedef: sizeof, and offsetof and sizeof of every field."""
    from upnerf_amd import _lib
    classes = abi_check.struct_classes(_lib)
    bad = abi_check.check_structs(classes, HEADER)
    assert not bad, "\n".join(bad)
    # the check looked at something: not fewer structs and fields than at the commit that introduced it
    assert len(classes) >= 61 and sum(len(c._fields_) for c in classes) >= 757


def test_every_signature_compiles_against_its_prototype():
    from upnerf_amd import _lib
    bad = abi_check.check_prototypes(_lib._SIGNATURES, _lib._LONGLONG, HEADER)
    assert not bad, "\n".join(bad)
    assert len(_lib._SIGNATURES) >= 98


def test_every_constant_of_the_header_is_mirrored_or_listed():
    from upnerf_amd import _lib
    bad = abi_check.check_constants(vars(_lib), HEADER, UNMIRRORED)
    assert not bad, "\n".join(bad)
    assert len(abi_check.constants(HEADER)) >= 39


MADE_UP = """#include <stdint.h>
#define UPNERF_MAX_THINGS 4
enum { UPNERF_KIND_A, UPNERF_KIND_B };
typedef struct { int32_t n, reserved_; const float* t0; const float* t1; float* out; } upnerf_span_args;
typedef struct { int32_t R, mode; const float* rgb; float* depth; } upnerf_shade_args;
typedef struct { const float* g; int32_t off, n; } upnerf_item_desc;
int upnerf_span(const upnerf_span_args* a, const float* rays, int n, void* stream);
long long upnerf_span_scratch(int n);
int upnerf_shade(const upnerf_shade_args* a, const upnerf_item_desc* items, int nitems, void* stream);
"""


def test_the_checker_reports_each_planted_error(tmp_path):
    """A three-struct header and its mirrors, with one error planted at a time: each is reported, by struct and field or by
    function.  (Neither the real header nor the library is touched.)"""
    from ctypes import POINTER, Structure, c_float, c_int, c_int32, c_void_p
    header = tmp_path / "upnerf_made_up.h"
    header.write_text(MADE_UP)
    i32, p = c_int32, c_void_p
    mirror = lambda name, *fields: type(name, (Structure,), {"_fields_": list(fields)})
    span = [("n", i32), ("reserved_", i32), ("t0", p), ("t1", p), ("out", p)]
    shade = [("R", i32), ("mode", i32), ("rgb", p), ("depth", p)]
    Span, Shade, Item = mirror("SpanArgs", *span), mirror("ShadeArgs", *shade), mirror("ItemDesc", ("g", p), ("off", i32), ("n", i32))
    structs = lambda *cls: abi_check.check_structs(cls, str(header))
    assert structs(Span, Shade, Item) == []
    swapped = mirror("SpanArgs", *span[:2], span[3], span[2], span[4])  # t1 before t0: what sizeof alone cannot see
    assert ctypes.sizeof(swapped) == ctypes.sizeof(Span)
    bad = structs(swapped, Shade, Item)
    assert len(bad) == 2 and "SpanArgs.t1" in bad[0] and "SpanArgs.t0" in bad[1], bad
    bad = structs(mirror("SpanArgs", *span[:4], ("dst", p)), Shade, Item)  # renamed: the compiler's message, and the name left out
    assert any("upnerf_span_args" in b and "dst" in b for b in bad) and "upnerf_span_args.out: not in the mirror SpanArgs" in bad, bad
    dropped = mirror("ShadeArgs", shade[0], *shade[2:])  # padding takes the place of `mode`: no size and no offset moves
    assert ctypes.sizeof(dropped) == ctypes.sizeof(Shade) and dropped.rgb.offset == Shade.rgb.offset
    assert structs(Span, dropped, Item) == ["upnerf_shade_args.mode: not in the mirror ShadeArgs"]
    assert structs(Span, Shade) == ["upnerf_item_desc: no ctypes class mirrors it"]
    assert structs(Span, Shade, Item, mirror("Extra", ("n", i32))) == ["Extra: the header has no typedef upnerf_extra"]

    good = {"upnerf_span": [POINTER(Span), POINTER(c_float), c_int, p], "upnerf_span_scratch": [c_int],
            "upnerf_shade": [POINTER(Shade), POINTER(Item), c_int, p]}
    protos = lambda longlong=("upnerf_span_scratch",), **over: abi_check.check_prototypes({**good, **over}, longlong, str(header))
    assert protos() == []
    for name, argtypes, what in (("upnerf_span", good["upnerf_span"][:3], "too few arguments"),                  # one short
                                 ("upnerf_span", [POINTER(Span), c_int, c_int, p], "pointer from integer"),     # pointer as c_int
                                 ("upnerf_shade", [POINTER(Shade), POINTER(Span), c_int, p], "incompatible pointer")):
        bad = protos(**{name: argtypes})
        assert len(bad) == 1 and bad[0].startswith(name + ": ") and what in bad[0], bad
    bad = protos(longlong=())  # the 64-bit return bound as int: by the set, and by the narrowing assignment
    assert len(bad) == 2 and all(b.startswith("upnerf_span_scratch: ") for b in bad), bad

    consts = dict(MAX_THINGS=4, KIND_A=0, KIND_B=1)
    assert abi_check.check_constants(consts, str(header), ()) == []
    bad = abi_check.check_constants({**consts, "MAX_THINGS": 5}, str(header), ())
    assert len(bad) == 1 and bad[0].startswith("MAX_THINGS: 5 in Python") and "is 4" in bad[0], bad
    assert len(abi_check.check_constants({"MAX_THINGS": 4, "KIND_A": 0}, str(header), ())) == 1  # KIND_B: neither mirrored nor listed
    assert len(abi_check.check_constants(consts, str(header), ("KIND_B",))) == 1  # listed as unmirrored, yet mirrored


def test_missing_library_fails_loudly(tmp_path, monkeypatch):
    import upnerf_amd._lib as L
    monkeypatch.setattr(L, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(ImportError):
        L._load()


def test_argument_errors_are_reported_not_crashed():
    from upnerf_amd import _lib
    assert _lib.lib.upnerf_sort_rows(0, 4, None, None) == -1
    assert _lib.lib.upnerf_linear(4, 4, 7, None, 0, None, 0, None, None, 0, 0, None) == -1
    L = _lib.Layout()
    L.W, L.D, L.skip = 100, 8, 4
    assert _lib.lib.upnerf_field_fwd(ctypes.byref(L), ctypes.byref(_lib.FieldFwdArgs()), None) == -2
    # the register-resident kernels write whole 256-sample tiles: a caller that states how many rows its tensors have is refused
    # when that is less than ceil(M / 256) * 256 (r4 ADVICE) -- before anything is launched
    L.W, L.D, L.skip = 256, 8, 4
    one = ctypes.cast(ctypes.c_void_p(16), ctypes.c_void_p)  # (non-null, never dereferenced on the host)
    fa = _lib.FieldFwdArgs(R=10, S=64, planes=1, tile_rows=256, rays_o=one, rays_d=one, z=one, P=one, P16=one, wexp=one, x0=one,
                           sigma_s=one, wnorm=one, rows_capacity=640)
    assert _lib.lib.upnerf_field_fwd_f16x3(ctypes.byref(L), ctypes.byref(fa), None) == -1  # 640 rows < 768


def _wgrad_desc(a=None, b=None, **kw):
    """A upnerf_wgrad_desc that upnerf_wgrad16 would launch: 256 x 256 from fp32 rows, every pointer set (non-null, never
    dereferenced: each case below is refused on the host).  a / b: fields of the two operands, kw: fields of the descriptor."""
    from upnerf_amd import _lib
    one = ctypes.c_void_p(16)
    op = lambda f: _lib.WgradOperand(**{**dict(p=one, lo=one, exp=one, ld=256, kind=_lib.WG_F32), **(f or {})})
    d = _lib.WgradDesc(M=512, N=256, K=256, planes=2, A=op(a), B=op(b), expo_a=one, expo_b=one, dW=one, db=one, ldo=256, nsplit=2,
                       slabs=one)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _wg_kinds():
    from upnerf_amd import _lib
    return _lib.WG_F32, _lib.WG_F16_TILE, _lib.WG_F16_FRAG, _lib.WG_F24, _lib.WG_PLANES


F32, TILE, FRAG, F24, PLANES = range(5)  # UPNERF_WG_* (checked against _lib below)
EINVAL, EUNSUP = -1, -2
# one row per refusal of upnerf_wgrad16, each reachable through one of the nine entry points it replaced (named on the right)
WGRAD_REFUSALS = [
    # null pointers and empty sizes
    (None, None, dict(M=0), EINVAL), (None, None, dict(nsplit=0), EINVAL), (dict(p=None), None, {}, EINVAL), (None, dict(p=None), {}, EINVAL),
    (None, None, dict(dW=None), EINVAL), (None, None, dict(slabs=None), EINVAL), (None, None, dict(expo_a=None), EINVAL),
    (None, None, dict(expo_b=None), EINVAL),
    (dict(kind=TILE, exp=None), dict(kind=TILE), {}, EINVAL),                 # f16p: A16 without its exponents
    (None, None, dict(v=16, dv=None), EINVAL),                                # f16x3_chain_v: a riding head without its destination
    (dict(kind=F24, lo=None), dict(kind=F24), {}, EINVAL),                    # f24p_chain: no residual bytes for A
    (dict(kind=PLANES, lo=None), dict(kind=PLANES), {}, EINVAL),              # planes_chain: a missing lo plane
    (dict(kind=PLANES), dict(kind=PLANES, lo=None), {}, EINVAL),
    # alignment: & 3 for fp32 operands, & 7 for fp16 operands, ldo & 3
    (dict(ld=258), None, {}, EINVAL), (None, dict(ld=258), {}, EINVAL), (None, None, dict(N=254), EINVAL), (None, None, dict(K=62), EINVAL),
    (None, None, dict(ldo=258), EINVAL),
    (dict(kind=TILE, ld=260), dict(kind=TILE), {}, EINVAL), (dict(kind=TILE), dict(kind=TILE, ld=260), {}, EINVAL),
    (dict(kind=TILE), dict(ld=68), dict(K=64), EINVAL),                       # (a fp32 B beside fp16 A is held to 8 as well)
    (dict(kind=TILE), dict(kind=TILE), dict(ldo=258), EINVAL), (dict(kind=PLANES), dict(kind=PLANES), dict(ldo=258), EINVAL),
    # planes outside {0, 1, 2}
    (None, None, dict(planes=3), EINVAL), (None, None, dict(planes=-1), EINVAL),
    # bad n2 / dW2 / ldo2
    (None, None, dict(n2=-1), EINVAL), (None, None, dict(n2=256), EINVAL), (None, None, dict(n2=128, dW2=None, ldo2=256), EINVAL),
    (None, None, dict(n2=128, dW2=16, ldo2=258), EINVAL), (dict(kind=FRAG), dict(kind=FRAG), dict(n2=128, dW2=None, ldo2=256), EINVAL),
    # a fp16 B without exp
    (dict(kind=TILE), dict(kind=TILE, exp=None), {}, EINVAL), (dict(kind=FRAG), dict(kind=FRAG, exp=None), {}, EINVAL),
    # F24 A with fragment order, or a fp16 F24 B without lo
    (dict(kind=F24), dict(kind=FRAG), {}, EINVAL), (dict(kind=F24), dict(kind=F24, lo=None), {}, EINVAL),
    # a riding head on anything but N = K = 256 with planes == 2 rows or fragment operands
    (None, None, dict(v=16, dv=16, planes=1), EUNSUP), (None, None, dict(v=16, dv=16, planes=0), EUNSUP),
    (None, None, dict(v=16, dv=16, N=128), EUNSUP), (None, None, dict(v=16, dv=16, K=64), EUNSUP),
    # PLANES with M & 63
    (dict(kind=PLANES), dict(kind=PLANES), dict(M=528), EUNSUP),
    # fragment shapes other than 256 / 128 with K = N, or fp32 B with N = 256
    (dict(kind=FRAG), dict(kind=FRAG), dict(N=64, K=64), EUNSUP), (dict(kind=FRAG), dict(kind=FRAG), dict(N=256, K=128), EUNSUP),
    (dict(kind=FRAG), dict(ld=64), dict(N=128, K=64), EUNSUP),
    # any block shape a packed kind has no instantiation for
    (dict(kind=TILE), dict(kind=TILE), dict(N=128, K=128), EUNSUP), (dict(kind=TILE), dict(kind=TILE), dict(K=64), EUNSUP),
    (dict(kind=TILE), None, {}, EUNSUP),                                      # (fp32 B: 256 x 64 only)
    (dict(kind=FRAG), dict(ld=128), dict(K=128), EUNSUP),
    (dict(kind=F24), dict(kind=F24), dict(N=128, K=128), EUNSUP), (dict(kind=F24), None, dict(K=128), EUNSUP),
]


@pytest.mark.parametrize("a,b,kw,want", WGRAD_REFUSALS)
def test_wgrad16_refuses_before_launch(a, b, kw, want):
    from upnerf_amd import _lib
    assert _wg_kinds() == (F32, TILE, FRAG, F24, PLANES)
    d = _wgrad_desc(a, b, **kw)
    assert _lib.lib.upnerf_wgrad16(ctypes.byref(d), None, None) == want
    assert _lib.lib.upnerf_wgrad16(ctypes.byref(d), ctypes.byref(_lib.WgradPending()), None) == want  # as a link of a run too


def test_wgrad16_refuses_the_slabs_that_are_still_pending():
    from upnerf_amd import _lib
    d = _wgrad_desc()
    pend = _lib.WgradPending(nsplit=2, slabs=d.slabs, rblocks=1)
    assert _lib.lib.upnerf_wgrad16(ctypes.byref(d), ctypes.byref(pend), None) == EINVAL
    assert _lib.lib.upnerf_wgrad16(None, None, None) == EINVAL


@pytest.mark.parametrize("N,K,tile", [(256, 256, (256, 256)), (256, 64, (256, 64)), (128, 128, (128, 128)), (128, 256, (128, 256))])
@pytest.mark.parametrize("nsplit", [1, 3])
@pytest.mark.parametrize("v", [False, True])
def test_wgrad16_scratch_is_the_closed_form_of_the_carve_up(N, K, tile, nsplit, v):
    """nsplit * (gy gz TN TK + gy TN) floats of slabs and bias slabs, plus nsplit * (K + 4) for a riding head; not less than the
    constants the Python side used to allocate for a 256 x 256 problem (with a riding head: + 260 per split)."""
    from upnerf_amd import _lib
    TN, TK = tile
    gy, gz = -(-N // TN), -(-K // TK)
    d = _wgrad_desc(N=N, K=K, nsplit=nsplit, v=16 if v else None)
    got = _lib.lib.upnerf_wgrad16_scratch(ctypes.byref(d))
    assert got == nsplit * (gy * gz * TN * TK + gy * TN) + (nsplit * (K + 4) if v else 0)
    if (N, K) == (256, 256):
        assert got >= nsplit * (256 * 256 + 256 + 260 if v else 256 * 256 + 256)
    assert _lib.lib.upnerf_wgrad16_scratch(ctypes.byref(_wgrad_desc(nsplit=0))) == EINVAL


def _composite_args(kind, **kw):
    """Composite argument structs with every pointer set (non-null, never dereferenced: each case below is refused on the host)."""
    from upnerf_amd import _lib
    cls = _lib.CompositeFwdArgs if kind == "fwd" else _lib.CompositeBwdArgs
    one = ctypes.c_void_p(16)
    a = cls(**{n: one for n, t in cls._fields_ if t is not ctypes.c_int32})
    a.R, a.S, a.W, a.mode, a.has_rgb = 5, 64, 64, 0, 1
    a.e16 = a.eexp = a.g2_16 = a.g2exp = None
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("kind", ["fwd", "bwd"])
@pytest.mark.parametrize("case,want", [
    (dict(S=0), -1), (dict(S=1025), -1), (dict(R=0), -1), (dict(W=128), -2), (dict(mode=4), -1), (dict(mode=-1), -1),
    # e as fp16 fragments needs W = 256 (the backward refuses it whether or not g_E_s is given)
    (dict(e16=16, eexp=16, g_E_s=None), -1), (dict(e16=16, eexp=16), -1),
    (dict(W=256, g2_16=16, g2exp=16), -1),  # g2 fragments without e16
])
def test_composite_argument_errors_are_refused_before_launch(kind, case, want):
    from upnerf_amd import _lib
    if kind == "fwd":
        case = {k: v for k, v in case.items() if k != "g_E_s"}
    a = _composite_args(kind, **case)
    fn = _lib.lib.upnerf_composite_fwd if kind == "fwd" else _lib.lib.upnerf_composite_bwd
    assert fn(ctypes.byref(a), None) == want


def test_ray_reduction_argument_errors_are_refused_before_launch():
    from upnerf_amd import _lib
    one = ctypes.c_void_p(16)
    assert _lib.lib.upnerf_ray_sum(4, 8, one, 257, one, None) == -1  # one thread per column, 256 at most
    assert _lib.lib.upnerf_ray_sum(4, 8, one, 0, one, None) == -1
    assert _lib.lib.upnerf_ray_sum(4, 0, one, 3, one, None) == -1
    assert _lib.lib.upnerf_ray_sum(0, 8, one, 3, one, None) == -1
    assert _lib.lib.upnerf_ray_geom_bwd(0, 8, one, one, one, one, None) == -1
    assert _lib.lib.upnerf_ray_geom_bwd(4, 0, one, one, one, one, None) == -1


def test_host_wrappers_refuse_or_fall_back_cleanly_without_a_gpu():
    """Host-side guards of the newer entry points: the sampler has no CPU path (raises), the embedding helper hands CPU
    tables to the module itself, the optimiser factory keeps torch.optim.Adam for CPU parameters."""
    import torch
    from upnerf_amd.ops import embed_rows
    from upnerf_amd.optim import FlatAdam, get_optimizer
    from upnerf_amd.ray_sampler import GpuRaySampler
    with pytest.raises(RuntimeError):
        GpuRaySampler(torch.zeros(4, 3), torch.zeros(4, 3), torch.zeros(4, 3), torch.zeros(1, 3, 4), device="cpu")
    emb = torch.nn.Embedding(5, 3)
    idx = torch.tensor([4, 0, 4])
    rows = embed_rows(emb, idx)
    assert torch.equal(rows, emb(idx))
    rows.sum().backward()
    assert emb.weight.grad is not None and float(emb.weight.grad[4].sum()) == 6.0
    lin = torch.nn.Linear(3, 2)
    opt = get_optimizer("adam", 1e-3, [lin])
    assert isinstance(opt, torch.optim.Adam) and not isinstance(opt, FlatAdam)
    with pytest.raises(ValueError):
        FlatAdam(lin.parameters())


def test_no_inline_asm_reads_an_mfma_result_inside_the_hazard_window(tmp_path):
    """hipcc does not pad an MFMA-result -> VALU-read hazard when the reader is an inline-asm statement (stale
    lanes in a few rows per 65 536, different rows every run).  The rule of this code base -- inline asm (v_fma_mix_f32 in
    resid16 / mix16) only reads values that went through a compiler-visible vector instruction first -- is checked on the
    generated ISA: no v_fma_mix_f32 may read a register that a v_mfma wrote within the previous 12 instructions."""
    import re
    import shutil
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "upnerf_amd", "csrc")
    bad = []
    for src in ("field16.hip",):
        out = tmp_path / (src + ".s")
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-S",
                            "--cuda-device-only", os.path.join(csrc, src), "-o", str(out)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        window = []  # (first, last) destination registers of recent v_mfma, one entry per instruction slot
        n_mix = 0
        for line in open(out):
            t = line.strip()
            if not t or t.startswith((";", ".", "//")) or t.endswith(":"):
                continue
            op = t.split()[0]
            m = re.match(r"v_mfma\S*\s+v\[(\d+):(\d+)\]", t)
            if op == "s_nop":  # an s_nop N stands for N + 1 wait states
                window = (window + [None] * (int(t.split()[1]) + 1))[-12:]
                continue
            if op.startswith("v_fma_mix_f32"):
                n_mix += 1
                srcs = [int(x) for x in re.findall(r"v(\d+)", t.split(",", 1)[1])]
                for w in window:
                    if w and any(w[0] <= s <= w[1] for s in srcs):
                        bad.append((src, t))
            window = (window + [(int(m.group(1)), int(m.group(2))) if m else None])[-12:]
        assert n_mix > 100, (src, n_mix)  # the check looked at something
    assert not bad, bad[:5]
