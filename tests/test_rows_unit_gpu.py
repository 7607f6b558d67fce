"""The row kernels ALONE (vrag_debug_rows_run, csrc/norm_heads.hip: the six launchers) against float64 references of the
arithmetic csrc/norm_heads.h documents (tests/rows_ref.py), on the SAME fp32 input values the kernels read, at the hidden sizes
where the 1024-slot register row has one live lane, a full slot, one lane in the next slot and no padding at all, at row counts
off the four-rows-per-workgroup grid, in every output form.

Bound, per output element (rows_ref.ln_bound and friends; never tuned to what the kernels return).  U = 2^-24; g(n) = n U / (1 -
n U) is a chain of n roundings; "one ulp" = 2 U relative is granted to every division and square root (they are correctly
rounded as built; one ulp also covers a fused v_rsq_f32).  ex is what the input of a step is already off by.
  mean         the row sum passes at most 15 in-lane additions and 6 shuffle levels: g(21) sum |x| / H, the division one ulp:
               E_m = mean(ex) + g(21) sum(|x| + ex) / H + 2 U |mean|.
  d = x - mean one rounding, and it inherits E_m WHOLE: E_d = E_m + ex + U |d~|.  Scaled by rstd |w| this is the term that grows
               with |mean| / sigma: a row at 100 +- 0.01 has E_m ~ 1.4e-4, 1.4 % of sigma, and nothing in a two-pass fp32
               LayerNorm can do better than U |mean| / sigma.
  variance     sum d~^2 - sum d^2 = 2 sum d_i (e_i + rho_i) + sum (c + e_i + rho_i)^2 with c the common shift (|c| <= E_m), e_i the
               input error, rho_i the rounding of the subtraction: the first-order term in c vanishes because sum d = 0.  Each
               product (or fma) rounds and the sum is again 15 + 6 deep: g(23) sum (|d| + E_d)^2; / H one ulp.
  rstd         var + eps rounds once; with q = E_(var + eps) / (var + eps) (asserted < 1/2, true of every family used) the factor
               is within (1 - q)^-1/2 (1 + 4 U) - 1 =: e_r: sqrtf and 1 / x one ulp each.
  output       y0 = d rstd w: rstd |w| (E_d (1 + e_r) + |d| e_r), two multiplies g(2) |y0|; the bias add U |y|.
  16-bit store unit16.out16_bound: the fp32 bound plus half an ulp of the stored value.  Where the launch also returns the fp32
               row the stored bits are predictable: hi must BE RNE(out_f32) (reference = the rounded value; the nominal bound
               U |x| only keeps the ratio finite, the conversion has no fp32 rounding), and hi + lo is judged against out_f32
               with half an ulp of lo = out_f32 - hi (exact in fp32): twice the operand precision.  Without out_f32 the same two
               checks run against the float64 row with E_y added.
  gelu_erf     0.5f * x * (1.0f + erff(x * 0.70710678f)): the argument's product rounds and its constant is rounded, U each
               on z and |z erf'(z)| <= 0.4839; erff ERF_ULP ulp = 2 ERF_ULP U |erf|; 1 + erf rounds; two more multiplies (0.5 x is
               exact): 0.5 |x| (32 U |erf| + 0.97 U + U |1 + erf|) + U |gelu|; an input error passes with sup |gelu'| = 1.129.
  tanhf        TANH_ULP ulp = 2 TANH_ULP U |tanh|; an argument error passes with |tanh'| <= 1.
               erff and tanhf come from the device math library, whose accuracy this project cannot derive.  ERF_ULP = 16 and
               TANH_ULP = 5 are the single-precision limits of the OpenCL C specification (table "ULP values for single precision
               built-in math functions", full profile), which the ROCm device library is built to; the ROCm headers and documents
               installed beside the compiler state no figure of their own.  The measured share is in MEASURED.
  pooling      a wave adds at most k = ceil(n / 4) token rows, then the fixed 4-way LDS add: g(k + 3) sum_t |y_t|; 1 / n one
               ulp and one multiply: 3 U |v|.
  dot product  16 in-lane products and additions (or fmas) + 6 shuffle levels: g(23) sum |x| |w|, + sum ex |w|; the bias add
               U |logit|.  range_pool mode 1: q = sum v^2 the same way, sqrtf and the division one ulp each, one multiply.
  seq_head     phase 2 is judged on the pooled rows phase 1 RETURNED (an error of phase 1 is then not blamed on phase 2): each
               dense column is one fmaf chain of H steps from zero, g(H) sum |p| |Wd|; + bd U |z|; then gelu_erf, the LayerNorm
               and the dot product as above, each fed the error of the step before.
  embed_ln     (word + type) + position: each addition rounds, U |partial sum|, as ex of the LayerNorm.

Negative controls (float64 references with one defect, CPU, unmarked): each exceeds the bound 10 x on its named case.  One
cannot under the general bound and gets a crafted one: `hi` truncated instead of rounded is off by at most one ulp of hi and the
16-bit store is granted half of one, a ratio below 2.  Where the launch returns out_f32 the stored bits are known, so that
check's reference is RNE(out_f32) under the nominal bound above: the same check the GPU test runs (form "hi = RNE(out_f32)").

`-rP` prints the worst error / bound ratio per (op and form, H, type).  Measured on an MI355X: see MEASURED below."""
import ctypes as C
import itertools
import zlib

import numpy as np
import pytest

import verbatim_rag_amd  # noqa: F401
from verbatim_rag_amd import _lib
import rows_ref as R
from unit16 import U, f32, from16, half_ulp, make_ledger, out16_bound, to16

gpu = pytest.mark.gpu

MEASURED = """NOT MEASURED: no MI355X run of this module has been recorded yet (`-rP` prints the table: the worst error / bound ratio per
(op and form, H, type), the erff share in the "gelu" forms, the tanhf share in "pooler_classifier"), and the NaN clamp question is
answered from the instruction's documented behaviour only, not from hardware.  Controls, worst ratio on the named case (CPU):
variance over H - 1 317, eps outside the root 7794, one-pass fp32 variance 92374, padding in the variance 16050, gain first 6.8e5,
tanh GELU 120, `end` exclusive >= 43724, mean-then-LayerNorm >= 2.0e5, tail tokens dropped >= 35946, cls row + 1 2.6e6, position
from the row index 9.3e5, type row 0 8.4e5, split3 as [hi | hi | lo] 1.4e8 (fp16) / 3.5e9 (bf16), hi truncated 16373 (fp16) /
1.3e5 (bf16), pooler without tanh 3926, classifier bias omitted >= 837."""

EPS = 1e-5
HS = [4, 12, 252, 256, 260, 384, 768, 1020, 1024]
HS_SUB = [4, 260, 768, 1024]
ROWS = [1, 3, 4, 5, 9]
FAMILIES = ["unit", "offset", "const"]
EXTRA = 3                                   # canary rows behind `rows` in every output
CAN32 = np.uint32(0x7A5C7A5C)
CAN16 = np.uint16(0x7A5C)
_WORST, record, control = make_ledger()
DT = ("bf16", "fp16")
IN_NAMES = ("h", "ids", "E", "P", "pos", "type_row", "type_ids", "w", "bias", "start", "end", "first_row", "seq_row", "seq_len",
            "Wp", "bp", "WdT", "bd", "wn", "bn", "Wc", "bc")


# ------------------------------------------------------------------ the hook
class Result:
    def __init__(self, status, args, outs, h, rows):
        self.status, self.launch_status, self.sat = status, args.launch_status, args.f16_saturated
        self.outs, self.h, self.rows = outs, h, rows

    def __getitem__(self, k):
        return self.outs[k][:self.rows]

    def canaries_intact(self, from_row=None):
        r = self.rows if from_row is None else from_row
        for name, o in self.outs.items():
            tail = o[r:]
            ok = np.all(tail.view(np.uint32) == CAN32) if o.dtype == np.float32 else np.all(tail == CAN16)
            assert ok, f"{name}: rows at or beyond {r} were written"


def raw_run(op, H, rows, want=(), out_cols=None, alias=False, h_rows=None, **kw):
    """One call of the hook.  Arrays in kw are inputs (by struct field name), scalars are struct fields; `want` names the outputs
    to allocate (canary-filled, rows + EXTRA rows); alias: h is the fp32 output."""
    dbg = _lib.load_debug()
    a = _lib.DebugRowsArgs()
    keep, outs, h_buf = [], {}, None
    out_rows = rows + EXTRA
    for name in IN_NAMES:
        v = kw.pop(name, None)
        if v is None:
            continue
        v = np.ascontiguousarray(v, np.int32 if name in ("ids", "pos", "type_ids", "start", "end", "first_row", "seq_row", "seq_len") else np.float32)
        if name == "h" and alias:
            v = v.copy()
        keep.append(v)
        setattr(a, name, v.ctypes.data)
        if name == "h":
            h_buf = v
            a.h_rows = v.shape[0] if h_rows is None else h_rows
    for name in want:
        cols = {"out_f32": out_cols or H, "out16": 3 * H if kw.get("split3") else H, "out_lo": H, "row_mean": 1, "pooled": H}[name]
        if name in ("out16", "out_lo"):
            o = np.full((out_rows, cols), CAN16, np.uint16)
        else:
            o = np.full((out_rows, cols), CAN32, np.uint32).view(np.float32)
        outs[name] = o
        setattr(a, name, o.ctypes.data)
    a.op, a.H, a.rows, a.out_rows, a.eps = kw.pop("op_code", _lib.DEBUG_ROWS_OPS[op]), H, rows, out_rows, EPS
    a.alias_f32 = int(alias)
    a.launch_status, a.f16_saturated = -1, -1
    for k, v in kw.items():
        setattr(a, k, v)
    status = dbg.vrag_debug_rows_run(C.byref(a), 0)
    res = Result(status, a, outs, h_buf, rows)
    del keep
    return res


def run(op, H, rows, **kw):
    res = raw_run(op, H, rows, **kw)
    if res.status == -2:   # VRAG_ERR_HIP: a failed launch or a clobbered canary: nothing more goes onto this device
        msg = _lib.load_debug().vrag_last_error()
        pytest.exit(f"vrag_debug_rows_run: {msg.decode() if msg else res.status}", returncode=3)
    _lib.check_debug("vrag_debug_rows_run", res.status)
    assert res.launch_status == 0
    res.canaries_intact()
    return res


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32 if x.dtype == np.float32 else x.dtype)


def rng_for(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def gain(rng, H):
    return f32(1.0 + 0.5 * rng.standard_normal(H))


def vec(rng, H, s=1.0):
    return f32(s * rng.standard_normal(H))


# ------------------------------------------------------------------ layernorm: every output form
def pairwise_cover(axes):
    """A small set of combinations in which every pair of values of every two axes occurs (greedy)."""
    names = list(axes)
    need = {(i, a, j, b) for i, j in itertools.combinations(range(len(names)), 2) for a in axes[names[i]] for b in axes[names[j]]}
    full = list(itertools.product(*axes.values()))
    chosen = []
    while need:
        best = max(full, key=lambda c: sum((i, c[i], j, c[j]) in need for i, j in itertools.combinations(range(len(names)), 2)))
        need -= {(i, best[i], j, best[j]) for i, j in itertools.combinations(range(len(names)), 2)}
        chosen.append(dict(zip(names, best)))
    return chosen


LN_AXES = {"gain": (0, 1), "bias": (0, 1), "gelu": (0, 1), "row_mean": (0, 1), "of": ("null", "alias", "separate"),
           "ob": ("none", "plain", "lo", "split3")}
LN_COMBOS = pairwise_cover(LN_AXES)


def test_layernorm_combinations_cover_every_pair():
    assert len(LN_COMBOS) <= 24
    for (i, a), (j, b) in itertools.combinations(LN_AXES.items(), 2):
        for x in a:
            for y in b:
                assert any(c[i] == x and c[j] == y for c in LN_COMBOS), (i, x, j, y)


def ln_inputs(H, family, rows, combo, seed):
    rng = rng_for("ln", H, family, rows, seed)
    h = R.make_rows(rng, family, rows + EXTRA, H)
    return h, (gain(rng, H) if combo["gain"] else None), (vec(rng, H) if combo["bias"] else None)


def check16(form, H, f16, hi_bits, lo_bits, of, y, ey):
    """The 16-bit forms of one launch: hi (and lo) against the fp32 row where the launch returned one, else the float64 row."""
    hi = from16(hi_bits, f16)
    record(form + " out16", H, f16, hi, y, out16_bound(y, ey, f16))
    if of is not None:
        of64 = of.astype(np.float64)
        record(form + " hi = RNE(out_f32)", H, f16, hi, from16(to16(of, f16), f16), U * np.abs(of64) + 1e-300)
    if lo_bits is not None:
        lo = from16(lo_bits, f16)
        if of is not None:
            record(form + " hi + lo vs out_f32", H, f16, hi + lo, of64, half_ulp(of64 - hi, f16))
        else:
            record(form + " hi + lo", H, f16, hi + lo, y, ey + half_ulp(np.abs(y - hi) + ey, f16))


def ln_launch(H, f16, combo, family, rows, seed=0):
    h, w, b = ln_inputs(H, family, rows, combo, seed)
    want = [n for n, on in (("out_f32", combo["of"] == "separate"), ("out16", combo["ob"] != "none"), ("out_lo", combo["ob"] == "lo"),
                            ("row_mean", combo["row_mean"])) if on]
    res = run("layernorm", H, rows, want=want, alias=combo["of"] == "alias", h=h, w=w, bias=b, gelu_first=combo["gelu"],
              split3=int(combo["ob"] == "split3"), f16=int(f16))
    return h, w, b, res


@gpu
@pytest.mark.parametrize("f16", (False, True), ids=DT)
@pytest.mark.parametrize("H", HS)
def test_layernorm(H, f16):
    for i, combo in enumerate(LN_COMBOS):
        family, rows = FAMILIES[(i + H) % 3], ROWS[(i + H // 4) % 5]
        h, w, b, res = ln_launch(H, f16, combo, family, rows)
        y, mean, ey, em = R.layernorm(h[:rows], w, b, EPS, bool(combo["gelu"]))
        form = "layernorm" + (" gelu" if combo["gelu"] else "")
        assert res.sat == 0
        of = None
        if combo["of"] == "separate":
            of = res["out_f32"]
        elif combo["of"] == "alias":
            of = res.h[:rows]
            assert np.array_equal(bits(res.h[rows:]), bits(h[rows:])), "the in-place launch wrote rows beyond `rows`"
        if of is not None:
            record(form + " out_f32", H, f16, of, y, ey)
        if combo["row_mean"]:
            record(form + " row_mean", H, f16, res["row_mean"][:, 0], mean, em)
        if combo["ob"] != "none":
            o = res["out16"]
            lo = res["out_lo"] if combo["ob"] == "lo" else o[:, H:2 * H] if combo["ob"] == "split3" else None
            if combo["ob"] == "split3":
                assert np.array_equal(o[:, :H], o[:, 2 * H:]), "[hi | lo | hi]: the two hi images differ"
            check16(form + (" split3" if combo["ob"] == "split3" else ""), H, f16, o[:, :H], lo, of, y, ey)


@gpu
@pytest.mark.parametrize("f16", (False, True), ids=DT)
def test_layernorm_in_place_equals_separate(f16):
    for H, rows in ((260, 5), (1024, 9), (4, 3)):
        base = {"gain": 1, "bias": 1, "gelu": 0, "row_mean": 1, "ob": "lo"}
        _, _, _, sep = ln_launch(H, f16, dict(base, of="separate"), "unit", rows)
        _, _, _, inp = ln_launch(H, f16, dict(base, of="alias"), "unit", rows)
        assert np.array_equal(bits(sep["out_f32"]), bits(inp.h[:rows]))
        for name in ("out16", "out_lo", "row_mean"):
            assert np.array_equal(bits(sep[name]), bits(inp[name])), name


@gpu
@pytest.mark.parametrize("f16", (False, True), ids=DT)
def test_layernorm_row_does_not_depend_on_its_batch(f16):
    """The same rows at other indices (another wave of the workgroup, another workgroup) among other neighbours: identical bits."""
    H = 260
    rng = rng_for("ln-indep", f16)
    a = R.make_rows(rng, "unit", 9, H)
    b = R.make_rows(rng, "offset", 13, H)
    where = [12, 3, 7, 0, 5, 10, 1, 6, 9]
    b[where] = a
    w, bias = gain(rng, H), vec(rng, H)
    kw = dict(want=["out_f32", "out16", "out_lo", "row_mean"], w=w, bias=bias, gelu_first=1, f16=int(f16))
    ra, rb = run("layernorm", H, 9, h=a, **kw), run("layernorm", H, 13, h=b, **kw)
    for name in kw["want"]:
        assert np.array_equal(bits(ra[name]), bits(rb[name][where])), name


# ------------------------------------------------------------------ embed_ln
EMBED_VARIANTS = ["modernbert", "bert types+bias", "bert type row 0"]


def embed_case(H, variant, family, rows, seed=0):
    rng = rng_for("embed", H, variant, family, rows, seed)
    vocab, n_pos, n_types = 37, 16, 2
    kw = {"E": R.make_rows(rng, family, vocab, H), "w": gain(rng, H), "vocab": vocab}
    ids = (np.arange(rows) * 17 + 5) % vocab                      # neighbouring rows gather distant embedding rows
    kw["ids"] = ids[rng.permutation(rows)] if rows > 1 else ids
    if variant != "modernbert":
        kw.update(P=vec(rng, H * n_pos, 0.3).reshape(n_pos, H), pos=rng.permutation(n_pos)[np.arange(rows) % n_pos], n_pos=n_pos,
                  type_row=vec(rng, H * n_types, 0.3).reshape(n_types, H), n_types=n_types)
        if variant == "bert types+bias":
            kw.update(type_ids=(np.arange(rows) + 1) % 2 if rows > 1 else np.ones(1, int), bias=vec(rng, H))
    return kw


def embed_ref(kw, defect=None):
    return R.embed_ln(np.asarray(kw["ids"]), kw["E"], kw["w"], EPS, kw.get("P"), kw.get("pos"), kw.get("type_row"), kw.get("type_ids"),
                      kw.get("bias"), defect)


@gpu
@pytest.mark.parametrize("f16", (False, True), ids=DT)
@pytest.mark.parametrize("H", HS)
def test_embed_ln(H, f16):
    i = 0
    for variant in EMBED_VARIANTS:
        for family in FAMILIES:
            rows = ROWS[(i + H // 4) % 5]
            i += 1
            kw = embed_case(H, variant, family, rows)
            res = run("embed_ln", H, rows, want=["out_f32", "out16"], f16=int(f16), **kw)
            y, ey = embed_ref(kw)
            assert res.sat == 0
            form = "embed_ln " + variant.split()[0]
            record(form + " out_f32", H, f16, res["out_f32"], y, ey)
            check16(form, H, f16, res["out16"], None, res["out_f32"], y, ey)


# ------------------------------------------------------------------ range_pool
RANGE_LENGTHS = [1, 2, 3, 4, 5, 8, 9, 33]
RANGE_STARTS = [10, 0, 5, 30, 8, 20, 3, 27]       # overlapping, out of order
ZERO_RANGE = (60, 61)                              # h[61] = -h[60]: the mean vector is exactly zero


def range_case(H, family, lnw, num_labels, seed=0):
    rng = rng_for("range", H, family, lnw, num_labels, seed)
    h = R.make_rows(rng, family, 64, H)
    h[61] = -h[60]
    start = RANGE_STARTS + [ZERO_RANGE[0]]
    end = [s + n - 1 for s, n in zip(RANGE_STARTS, RANGE_LENGTHS)] + [ZERO_RANGE[1]]
    assert max(end) < 64
    return dict(h=h, w=gain(rng, H) if lnw else None, start=np.asarray(start), end=np.asarray(end),
                Wc=vec(rng, num_labels * H, H ** -0.5).reshape(num_labels, H), bc=vec(rng, num_labels))


def check_ranges(form, H, got, refs):
    for r, (ref, bound) in enumerate(refs):
        if not np.any(bound):
            assert np.all(got[r] == 0.0), "a zero mean vector must give a zero output (the 1e-12 floor)"
        else:
            record(form, H, None, got[r], ref, bound)


@gpu
@pytest.mark.parametrize("H", HS_SUB)
def test_range_pool(H):
    i = 0
    for lnw in (True, False):
        for mode in (0, 1, 2):
            for num_labels in ((1, 2, 4, 5, 9) if mode == 0 else (1,)):
                family = FAMILIES[i % 3]
                i += 1
                kw = range_case(H, family, lnw, num_labels)
                n = len(kw["start"])
                res = run("range_pool", H, n, want=["out_f32"], out_cols=num_labels if mode == 0 else H, mode=mode, num_labels=num_labels, **kw)
                refs = R.range_pool(kw["h"], kw["w"], EPS, kw["start"], kw["end"], mode, kw["Wc"], kw["bc"])
                if mode == 1:
                    assert not np.any(refs[-1][1]) and np.any(refs[0][1])
                check_ranges(f"range_pool mode {mode}" + (" ln" if lnw else ""), H, res["out_f32"], refs)


@gpu
def test_range_pool_does_not_depend_on_its_batch():
    H = 260
    kw = range_case(H, "unit", True, 5)
    n = len(kw["start"])
    rng = rng_for("range-indep")
    h2 = R.make_rows(rng, "offset", 80, H)
    h2[16:80] = kw["h"]
    perm = rng.permutation(n)
    for mode, cols in ((0, 5), (1, H), (2, H)):
        a = run("range_pool", H, n, want=["out_f32"], out_cols=cols, mode=mode, num_labels=5, **kw)
        b = run("range_pool", H, n, want=["out_f32"], out_cols=cols, mode=mode, num_labels=5,
                **dict(kw, h=h2, start=kw["start"][perm] + 16, end=kw["end"][perm] + 16))
        assert np.array_equal(bits(a["out_f32"][perm]), bits(b["out_f32"]))


# ------------------------------------------------------------------ ln_classifier
def lncls_case(H, family, rows, num_labels, lnb, seed=0):
    rng = rng_for("lncls", H, family, rows, num_labels, lnb, seed)
    return dict(h=R.make_rows(rng, family, rows, H), w=gain(rng, H), bias=vec(rng, H) if lnb else None,
                Wc=vec(rng, num_labels * H, H ** -0.5).reshape(num_labels, H), bc=vec(rng, num_labels))


@gpu
@pytest.mark.parametrize("H", HS_SUB)
def test_ln_classifier(H):
    i = 0
    for num_labels in (1, 2, 7):
        for lnb in (False, True):
            for gelu in (0, 1):
                family, rows = FAMILIES[i % 3], ROWS[i % 5]
                i += 1
                kw = lncls_case(H, family, rows, num_labels, lnb)
                res = run("ln_classifier", H, rows, want=["out_f32"], out_cols=num_labels, num_labels=num_labels, gelu_first=gelu, **kw)
                ref, bound = R.ln_classifier(kw["h"], kw["w"], EPS, kw["Wc"], kw["bc"], kw["bias"], bool(gelu))
                record("ln_classifier" + (" gelu" if gelu else ""), H, None, res["out_f32"], ref, bound)


# ------------------------------------------------------------------ pooler_classifier
def pooler_case(H, family, n_seqs, num_labels, seed=0):
    rng = rng_for("pooler", H, family, n_seqs, num_labels, seed)
    first = np.asarray([11, 2, 19, 0, 7][:n_seqs])                # not ascending
    return dict(h=R.make_rows(rng, family, 20, H), first_row=first, Wp=vec(rng, H * H, H ** -0.5).reshape(H, H), bp=vec(rng, H),
                Wc=vec(rng, num_labels * H, H ** -0.5).reshape(num_labels, H), bc=vec(rng, num_labels))


@gpu
@pytest.mark.parametrize("H", HS_SUB)
def test_pooler_classifier(H):
    i = 0
    for n_seqs in (1, 5):
        for num_labels in (1, 2, 5):
            family = FAMILIES[i % 3]
            i += 1
            kw = pooler_case(H, family, n_seqs, num_labels)
            res = run("pooler_classifier", H, n_seqs, want=["out_f32"], out_cols=num_labels, num_labels=num_labels, **kw)
            ref, bound = R.pooler_classifier(kw["h"], kw["first_row"], kw["Wp"], kw["bp"], kw["Wc"], kw["bc"])
            record("pooler_classifier", H, None, res["out_f32"], ref, bound)


# ------------------------------------------------------------------ seq_head
SEQ_LENGTHS = [1, 2, 3, 4, 5, 12, 13, 16, 17, 28, 29, 33, 9, 6, 31, 20, 7]
SEQ_H_ROWS = 320


def seq_layout(n_seqs, seed=0):
    """Scattered, non-ascending first rows without overlap."""
    rng = rng_for("seq-layout", n_seqs, seed)
    lens = [SEQ_LENGTHS[(i + 3 * seed) % len(SEQ_LENGTHS)] for i in range(n_seqs)] if n_seqs < 12 else SEQ_LENGTHS[:n_seqs]
    row, cur = [0] * n_seqs, int(rng.integers(0, 3))
    for i in rng.permutation(n_seqs):
        row[i] = cur
        cur += lens[i] + int(rng.integers(0, 3))
    assert cur <= SEQ_H_ROWS
    return np.asarray(row), np.asarray(lens)


def seq_case(H, family, n_seqs, num_labels, bd, bn, seed=0):
    rng = rng_for("seq", H, family, n_seqs, num_labels, bd, bn, seed)
    row, lens = seq_layout(n_seqs, seed)
    return dict(h=R.make_rows(rng, family, SEQ_H_ROWS, H), w=gain(rng, H), seq_row=row, seq_len=lens,
                WdT=vec(rng, H * H, H ** -0.5).reshape(H, H), bd=vec(rng, H) if bd else None, wn=gain(rng, H),
                bn=vec(rng, H) if bn else None, Wc=vec(rng, num_labels * H, H ** -0.5).reshape(num_labels, H), bc=vec(rng, num_labels))


def seq_check(form, H, kw, res, pool_mean):
    pref, pbound = R.seq_pool(kw["h"], kw["w"], EPS, kw["seq_row"], kw["seq_len"], pool_mean)
    record(form + " pooled", H, None, res["pooled"], pref, pbound)
    ref, bound = R.seq_head_logits(res["pooled"], kw["WdT"], kw["bd"], kw["wn"], kw["bn"], EPS, kw["Wc"], kw["bc"])
    record(form + " logits", H, None, res["out_f32"], ref, bound)


@gpu
@pytest.mark.parametrize("H", HS_SUB)
def test_seq_head(H):
    i = 0
    for n_seqs in (1, 7, 8, 9, 17):
        for pool_mean in (0, 1):
            family, num_labels, bd, bn = FAMILIES[i % 3], (1, 3)[i % 2], bool(i & 1), bool(i & 2)
            i += 1
            kw = seq_case(H, family, n_seqs, num_labels, bd, bn)
            if not pool_mean:   # the first token alone may be read: everything else is NaN
                keep = kw["h"][kw["seq_row"]].copy()
                kw["h"][:] = np.nan
                kw["h"][kw["seq_row"]] = keep
            res = run("seq_head", H, n_seqs, want=["out_f32", "pooled"], out_cols=num_labels, num_labels=num_labels, mode=pool_mean, **kw)
            assert np.all(np.isfinite(res["pooled"])) and np.all(np.isfinite(res["out_f32"]))
            seq_check("seq_head " + ("mean" if pool_mean else "cls"), H, kw, res, pool_mean)
    # bd and bn each with and without the other, both label counts, on the full-length list
    for bd, bn, num_labels in ((False, False, 3), (True, False, 1), (False, True, 1), (True, True, 3)):
        kw = seq_case(H, "unit", 17, num_labels, bd, bn, seed=1)
        res = run("seq_head", H, 17, want=["out_f32", "pooled"], out_cols=num_labels, num_labels=num_labels, mode=1, **kw)
        seq_check("seq_head mean", H, kw, res, 1)


def test_seq_layouts_hold_every_length():
    row, lens = seq_layout(17)
    assert set(lens) >= {1, 2, 3, 4, 5, 12, 13, 16, 17, 28, 29, 33}
    assert list(row) != sorted(row)


@gpu
def test_seq_head_does_not_depend_on_its_batch():
    """A sequence's pooled row and logits at list index 2, 7 (last of a full block), 8 (first of the next) and 16 (alone in the
    third block), among other neighbours, and alone: identical bits."""
    H = 260
    for pool_mean in (0, 1):
        kw = seq_case(H, "unit", 17, 3, True, True, seed=2)
        alone = run("seq_head", H, 1, want=["out_f32", "pooled"], out_cols=3, num_labels=3, mode=pool_mean,
                    **dict(kw, seq_row=kw["seq_row"][11:12], seq_len=kw["seq_len"][11:12]))
        for at in (2, 7, 8, 16):
            order = np.arange(17)
            order[[at, 11]] = order[[11, at]]
            res = run("seq_head", H, 17, want=["out_f32", "pooled"], out_cols=3, num_labels=3, mode=pool_mean,
                      **dict(kw, seq_row=kw["seq_row"][order], seq_len=kw["seq_len"][order]))
            for name in ("pooled", "out_f32"):
                assert np.array_equal(bits(res[name][at:at + 1]), bits(alone[name])), (name, at, pool_mean)


# ------------------------------------------------------------------ refusals
def test_hook_refusals():
    """What the hook itself refuses comes before any GPU call: the argument error, a message of its own, nothing written."""
    H, rows = 8, 4
    rng = rng_for("refuse")
    h = R.make_rows(rng, "unit", 16, H)
    seen = set()

    def refused(op, want=("out_f32",), **kw):
        res = raw_run(op, kw.pop("H", H), kw.pop("rows", rows), want=list(want), **kw)
        assert res.status == -1 and res.launch_status == -1, (op, kw.keys(), res.status)
        res.canaries_intact(0)
        seen.add(_lib.load_debug().vrag_last_error().decode().split("(")[0].split("[")[0].rstrip("0123456789 -"))

    emb = dict(E=h, w=h[0], ids=np.arange(rows), vocab=16, want=("out_f32", "out16"))
    refused("embed_ln", **dict(emb, ids=None))
    refused("embed_ln", **dict(emb, want=("out_f32",)))
    refused("embed_ln", **dict(emb, ids=[0, 1, 16, 2]))
    refused("embed_ln", **dict(emb, ids=[0, -1, 3, 2]))
    refused("embed_ln", **dict(emb, P=h, pos=[0, 1, 2, 9], n_pos=9))
    refused("embed_ln", **dict(emb, P=h, pos=[0, 1, 2, 3], n_pos=9, type_row=h, n_types=2, type_ids=[0, 1, 2, 0]))
    refused("layernorm", h=None)
    refused("layernorm", h=h, rows=17)
    refused("layernorm", h=h, alias=True)                       # alias_f32 with out_f32
    refused("layernorm", h=h, out_rows=2)
    refused("layernorm", h=h, H=0)
    refused("layernorm", h=h, rows=-1)
    refused("layernorm", h=h, op_code=9)
    rp = dict(h=h, start=[0, 2, 4, 6], end=[1, 3, 5, 15], mode=2)
    refused("range_pool", **dict(rp, end=[1, 3, 5, 16]))
    refused("range_pool", **dict(rp, start=[0, -1, 4, 6]))
    refused("range_pool", **dict(rp, start=[0, 4, 4, 6]))       # start > end
    refused("range_pool", **dict(rp, end=None))
    refused("range_pool", **dict(rp, mode=0, Wc=h[:2], bc=h[0, :2], num_labels=0))
    refused("range_pool", **dict(rp, mode=0, bc=h[0, :2], num_labels=2))
    cls = dict(Wc=h[:2], bc=h[0, :2], num_labels=2)
    refused("ln_classifier", h=h, **cls)                         # no w
    refused("ln_classifier", h=h, w=h[0], **dict(cls, num_labels=0))
    pc = dict(h=h, Wp=h[:8], bp=h[0], first_row=[0, 3, 2, 15], **cls)
    refused("pooler_classifier", **dict(pc, first_row=[0, 3, 2, 16]))
    refused("pooler_classifier", **dict(pc, Wp=None))
    sh = dict(h=h, w=h[0], seq_row=[0, 4, 8, 12], seq_len=[4, 4, 4, 4], WdT=h[:8], wn=h[0], want=("out_f32", "pooled"), **cls)
    refused("seq_head", **dict(sh, seq_len=[4, 4, 4, 5]))
    refused("seq_head", **dict(sh, seq_len=[4, 0, 4, 4]))
    refused("seq_head", **dict(sh, seq_row=[0, -4, 8, 12]))
    refused("seq_head", **dict(sh, want=("out_f32",)))
    refused("seq_head", **dict(sh, num_labels=0))
    assert len(seen) >= 20, seen


@gpu
def test_launcher_refusals():
    """What the LAUNCHERS refuse reaches them through the hook unchecked: an error status, launch_status = hipErrorInvalidValue,
    every canary intact from row 0."""
    rng = rng_for("launcher-refuse")

    def refused(op, H, want, **kw):
        res = raw_run(op, H, 4, want=list(want), **kw)
        assert res.status == -1 and res.launch_status == 1, (op, H, res.status, res.launch_status)
        res.canaries_intact(0)
        assert res.sat == 0

    for H in (1028, 6):
        h = R.make_rows(rng, "unit", 16, H)
        cls = dict(Wc=h[:2], bc=h[0, :2], num_labels=2, out_cols=2)
        refused("layernorm", H, ("out_f32", "out16"), h=h, w=h[0])
        refused("embed_ln", H, ("out_f32", "out16"), E=h, w=h[0], ids=np.arange(4), vocab=16)
        refused("range_pool", H, ("out_f32",), h=h, start=[0, 1, 2, 3], end=[3, 3, 3, 3], mode=2)
        refused("ln_classifier", H, ("out_f32",), h=h, w=h[0], **cls)
        refused("pooler_classifier", H, ("out_f32",), h=h, first_row=[0, 1, 2, 3], Wp=np.zeros((H, H)), bp=h[0], **cls)
        refused("seq_head", H, ("out_f32", "pooled"), h=h, w=h[0], seq_row=[0, 4, 8, 12], seq_len=[4, 4, 4, 4], WdT=np.zeros((H, H)),
                wn=h[0], **cls)
    H = 8
    h = R.make_rows(rng, "unit", 16, H)
    cls = dict(Wc=h[:2], bc=h[0, :2], num_labels=2, out_cols=2)
    refused("layernorm", H, ("out16", "out_lo"), h=h, w=h[0], split3=1)
    refused("layernorm", H, ("out_f32",), h=h, w=h[0], split3=1)
    refused("layernorm", H, ("out_f32", "out16"), h=h, w=h[0], f16=1, no_sat=1)
    refused("embed_ln", H, ("out_f32", "out16"), E=h, w=h[0], ids=np.arange(4), vocab=16, f16=1, no_sat=1)
    refused("embed_ln", H, ("out_f32", "out16"), E=h, w=h[0], ids=np.arange(4), vocab=16, P=h, n_pos=16)
    refused("seq_head", H, ("out_f32", "pooled"), h=h, seq_row=[0, 4, 8, 12], seq_len=[4, 4, 4, 4], WdT=h[:8], wn=h[0], **cls)
    # rows = 0 is no error and no launch
    res = raw_run("layernorm", H, 0, want=["out_f32", "out16"], h=h, w=h[0])
    assert res.status == 0 and res.launch_status == 0
    res.canaries_intact(0)


# ------------------------------------------------------------------ the fp16 clamp word
def clamp_run(op, f16, H=260, rows=5, w_scale=1.0, poison=None, bias_inf=False):
    rng = rng_for("clamp", op)
    x = R.make_rows(rng, "unit", 16, H)
    w = f32(gain(rng, H) * w_scale)
    bias = vec(rng, H)
    if bias_inf:
        bias[7] = np.inf
    if poison is not None:
        x[2, 9] = poison
    if op == "layernorm":
        return x, run(op, H, rows, want=["out_f32", "out16"], h=x, w=w, bias=bias, f16=int(f16))
    return x, run(op, H, rows, want=["out_f32", "out16"], E=x, ids=np.arange(rows), vocab=16, w=w, bias=bias, f16=int(f16))


@gpu
@pytest.mark.parametrize("op", ("layernorm", "embed_ln"))
def test_fp16_clamp_word(op):
    _, res = clamp_run(op, True, w_scale=1e6)
    big = np.abs(res["out_f32"]) > 65504.0
    assert big.any() and res.sat == 1
    got = from16(res["out16"], True)
    assert np.array_equal(got[big], np.sign(res["out_f32"][big]) * 65504.0), "an out-of-range value is stored as +-65504"
    assert np.array_equal(res["out16"][~big], to16(res["out_f32"][~big], True))
    _, res = clamp_run(op, False, w_scale=1e6)
    assert res.sat == 0, "bf16 never clamps"
    assert np.array_equal(res["out16"], to16(res["out_f32"], False))
    _, res = clamp_run(op, True)
    assert res.sat == 0, "a healthy fp16 launch set the clamp word"
    _, res = clamp_run(op, True, bias_inf=True)
    assert np.all(np.isposinf(res["out_f32"][:, 7])) and res.sat == 1, "+inf is outside fp16's range"
    assert np.all(from16(res["out16"][:, 7], True) == 65504.0)


@gpu
@pytest.mark.parametrize("op", ("layernorm", "embed_ln"))
@pytest.mark.parametrize("poison", (np.nan, np.inf), ids=("nan", "inf-in-row"))
def test_fp16_clamp_word_on_nan(op, poison):
    """A NaN activation (or a +inf one, which the LayerNorm turns into a row of NaN) must set the clamp word: the fp32 row shows
    NaN, the 16-bit operand that feeds the next GEMM holds a finite value (what v_med3_f32 returns for a NaN operand)."""
    _, res = clamp_run(op, True, poison=poison)
    assert np.all(np.isnan(res["out_f32"][2])) and not np.any(np.isnan(res["out_f32"][[0, 1, 3, 4]]))
    stored = sorted({hex(int(v)) for v in res["out16"][2]})
    print(f"\n{op}: fp16 bits stored for a NaN row: {stored}")
    assert res.sat == 1, f"a NaN row was stored as {stored} and the clamp word stayed 0"
    _, res = clamp_run(op, False, poison=poison)
    assert res.sat == 0 and np.all(np.isnan(from16(res["out16"][2], False)))


# ------------------------------------------------------------------ CPU: the references against independent formulations
def test_references_against_torch_float64():
    torch = pytest.importorskip("torch")
    F = torch.nn.functional
    rng = rng_for("torch")
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    for H in (4, 260, 1024):
        for family in FAMILIES:
            x = R.make_rows(rng, family, 7, H)
            w, b = gain(rng, H), vec(rng, H)
            y, mean, _, _ = R.layernorm(x, w, b, EPS)
            assert np.allclose(y, F.layer_norm(t(x), (H,), t(w), t(b), EPS).numpy(), rtol=1e-9, atol=1e-9)
            assert np.allclose(mean, x.astype(np.float64).mean(1), rtol=1e-13)
            y, _, _, _ = R.layernorm(x, None, None, EPS, gelu_first=True)
            assert np.allclose(y, F.layer_norm(F.gelu(t(x)), (H,), None, None, EPS).numpy(), rtol=1e-9, atol=1e-9)
            # embed_ln against F.embedding and the sums in torch
            kw = embed_case(H, "bert types+bias", family, 9)
            e = F.embedding(torch.from_numpy(kw["ids"]), t(kw["E"])) + t(kw["type_row"])[torch.from_numpy(kw["type_ids"])] + t(kw["P"])[torch.from_numpy(kw["pos"])]
            assert np.allclose(embed_ref(kw)[0], F.layer_norm(e, (H,), t(kw["w"]), t(kw["bias"]), EPS).numpy(), rtol=1e-9, atol=1e-9)
            # range_pool: modes 1 and 0 against F.normalize / F.linear of the mean of F.layer_norm
            kw = range_case(H, family, True, 3)
            ln = F.layer_norm(t(kw["h"]), (H,), t(kw["w"]), None, EPS)
            refs1 = R.range_pool(kw["h"], kw["w"], EPS, kw["start"], kw["end"], 1)
            refs0 = R.range_pool(kw["h"], kw["w"], EPS, kw["start"], kw["end"], 0, kw["Wc"], kw["bc"])
            for r, (s, e_) in enumerate(zip(kw["start"][:-1], kw["end"][:-1])):
                v = ln[s:e_ + 1].mean(0)
                assert np.allclose(refs1[r][0], F.normalize(v, dim=0, eps=1e-12).numpy(), rtol=1e-9, atol=1e-12)
                assert np.allclose(refs0[r][0], F.linear(v, t(kw["Wc"]), t(kw["bc"])).numpy(), rtol=1e-9, atol=1e-9)
            # pooler and the sequence head
            kw = pooler_case(H, family, 5, 2)
            ref, _ = R.pooler_classifier(kw["h"], kw["first_row"], kw["Wp"], kw["bp"], kw["Wc"], kw["bc"])
            want = F.linear(torch.tanh(F.linear(t(kw["h"])[torch.from_numpy(kw["first_row"])], t(kw["Wp"]), t(kw["bp"]))), t(kw["Wc"]), t(kw["bc"]))
            assert np.allclose(ref, want.numpy(), rtol=1e-9, atol=1e-9)
            kw = seq_case(H, family, 9, 3, True, True)
            pooled, _ = R.seq_pool(kw["h"], kw["w"], EPS, kw["seq_row"], kw["seq_len"], 1)
            ln = F.layer_norm(t(kw["h"]), (H,), t(kw["w"]), None, EPS)
            want = torch.stack([ln[r:r + n].mean(0) for r, n in zip(kw["seq_row"], kw["seq_len"])])
            assert np.allclose(pooled, want.numpy(), rtol=1e-9, atol=1e-9)
            ref, _ = R.seq_head_logits(f32(pooled), kw["WdT"], kw["bd"], kw["wn"], kw["bn"], EPS, kw["Wc"], kw["bc"])
            z = F.gelu(F.linear(t(f32(pooled)), t(kw["WdT"]).T, t(kw["bd"])))
            want = F.linear(F.layer_norm(z, (H,), t(kw["wn"]), t(kw["bn"]), EPS), t(kw["Wc"]), t(kw["bc"]))
            assert np.allclose(ref, want.numpy(), rtol=1e-9, atol=1e-9)


# ------------------------------------------------------------------ CPU: negative controls
def test_layernorm_controls():
    def ln(H, family, defect, combo=None, gelu=False):
        h, w, b = ln_inputs(H, family, 9, combo or {"gain": 1, "bias": 1}, 0)
        y, _, ey, _ = R.layernorm(h[:9], w, b, EPS, gelu)
        wrong, _, _, _ = R.layernorm(h[:9], w, b, EPS, gelu, defect)
        return wrong, y, ey

    control("variance over H - 1 (unit rows, H = 1024)", *ln(1024, "unit", "var_H-1"))
    control("eps outside the square root (near-constant rows, H = 768)", *ln(768, "const", "eps_outside"))
    control("one-pass variance in fp32 (mean-offset rows, H = 768)", *ln(768, "offset", "one_pass_f32"))
    control("padding slots counted in the variance (H = 260)", *ln(260, "unit", "padding_in_var"))
    control("gain applied before the normalisation (H = 384)", *ln(384, "unit", "gain_first"))
    control("tanh-approximation GELU (gelu_first, H = 768)", *ln(768, "unit", "gelu_tanh", gelu=True))


@pytest.mark.parametrize("f16", (False, True), ids=DT)
def test_split_image_controls(f16):
    h, w, b = ln_inputs(260, "unit", 9, {"gain": 1, "bias": 1}, 0)
    y, _, ey, _ = R.layernorm(h[:9], w, b, EPS)
    of = f32(y)                                            # stands for the fp32 row a launch returns
    of64 = of.astype(np.float64)
    hi, lo = R.split_hi_lo(of, f16)
    image, wrong = R.split3_image(hi, lo), R.split3_image(hi, lo, "split3_weight_order")
    b16 = out16_bound(y, ey, f16)
    control(f"split3 as [hi | hi | lo] [{DT[f16]}]", wrong, np.concatenate([y, of64 - hi, y], -1),
            np.concatenate([b16, half_ulp(of64 - hi, f16), b16], -1))
    assert np.all(np.abs(image - np.concatenate([y, of64 - hi, y], -1)) <= np.concatenate([b16, half_ulp(of64 - hi, f16), b16], -1))
    hi_t, _ = R.split_hi_lo(of, f16, "hi_trunc")
    assert np.max(np.abs(hi_t - y) / b16) < 2.5            # why the crafted check exists
    control(f"hi truncated instead of rounded [{DT[f16]}]", hi_t, hi, U * np.abs(of64) + 1e-300)


def test_embed_controls():
    kw = embed_case(260, "bert types+bias", "unit", 9)
    y, ey = embed_ref(kw)
    control("position row from the row index instead of pos", embed_ref(kw, "pos_from_row")[0], y, ey)
    control("type row 0 instead of type_ids", embed_ref(kw, "type_row0")[0], y, ey)


def test_pool_controls():
    kw = range_case(260, "unit", True, 5)
    sel = [i for i, n in enumerate(RANGE_LENGTHS) if n >= 2]
    ref = R.range_pool(kw["h"], kw["w"], EPS, kw["start"][sel], kw["end"][sel], 2)
    for name, defect in (("`end` exclusive", "end_exclusive"), ("mean-then-LayerNorm", "mean_then_ln")):
        wrong = R.range_pool(kw["h"], kw["w"], EPS, kw["start"][sel], kw["end"][sel], 2, defect=defect)
        for (w_, _), (r_, b_), i in zip(wrong, ref, sel):
            control(f"{name} (range of {RANGE_LENGTHS[i]})", w_, r_, b_)
    kw = seq_case(260, "unit", 17, 3, True, True)
    tail = np.asarray([i for i, n in enumerate(kw["seq_len"]) if n % 4 and n > 4])
    args = (kw["h"], kw["w"], EPS, kw["seq_row"][tail], kw["seq_len"][tail])
    ref, bound = R.seq_pool(*args, 1)
    for i in range(len(tail)):
        control(f"last n % 4 tokens dropped (n = {kw['seq_len'][tail[i]]})", R.seq_pool(*args, 1, "drop_tail")[0][i], ref[i], bound[i])
    ref, bound = R.seq_pool(*args, 0)
    control("cls pooling takes row seq_row + 1", R.seq_pool(*args, 0, "cls_row+1")[0], ref, bound)


def test_head_controls():
    kw = pooler_case(260, "unit", 5, 2)
    args = (kw["h"], kw["first_row"], kw["Wp"], kw["bp"], kw["Wc"], kw["bc"])
    ref, bound = R.pooler_classifier(*args)
    control("pooler without tanh", R.pooler_classifier(*args, "no_tanh")[0], ref, bound)
    control("pooler: classifier bias omitted", R.pooler_classifier(*args, "no_cls_bias")[0], ref, bound)
    kw = lncls_case(260, "unit", 5, 2, True)
    args = (kw["h"], kw["w"], EPS, kw["Wc"], kw["bc"], kw["bias"])
    ref, bound = R.ln_classifier(*args, True)
    control("ln_classifier: classifier bias omitted", R.ln_classifier(*args, True, "no_cls_bias")[0], ref, bound)
    kw = seq_case(260, "unit", 9, 3, True, True)
    pooled = f32(R.seq_pool(kw["h"], kw["w"], EPS, kw["seq_row"], kw["seq_len"], 1)[0])
    args = (pooled, kw["WdT"], kw["bd"], kw["wn"], kw["bn"], EPS, kw["Wc"], kw["bc"])
    ref, bound = R.seq_head_logits(*args)
    control("seq_head: classifier bias omitted", R.seq_head_logits(*args, "no_cls_bias")[0], ref, bound)
    kw = range_case(260, "unit", True, 5)
    ref = R.range_pool(kw["h"], kw["w"], EPS, kw["start"], kw["end"], 0, kw["Wc"], kw["bc"])
    wrong = R.range_pool(kw["h"], kw["w"], EPS, kw["start"], kw["end"], 0, kw["Wc"], kw["bc"], "no_cls_bias")
    control("range_pool: classifier bias omitted", wrong[3][0], ref[3][0], ref[3][1])


# ------------------------------------------------------------------ the -rP table
@gpu
def test_zz_worst_ratios():
    print("\nworst error / bound per (op and form, H, type)")
    for (form, H, f16), r in sorted(_WORST.items(), key=lambda kv: (kv[0][0], kv[0][1] or 0, bool(kv[0][2]))):
        tag = "" if f16 is None else DT[bool(f16)]
        print(f"  {form:<58s} {str(H or ''):>5s} {tag:>5s} {r:10.4g}")
    for (form, H, f16), r in _WORST.items():
        if not form.startswith("control"):
            assert r <= 1.0, (form, H, f16, r)
