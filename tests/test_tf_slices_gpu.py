"""The transformer kernels, every family, per SLICE of every tensor and away from initialisation statistics (EXPERIMENTS 5.13).

Inputs: tests/tf_refs.py::trained_like — peaked softmax (logit std 3, mean largest probability 0.4, dominant keys planted in the first and in
the last key tile), LayerNorm gains of mixed sign up to 3, biases everywhere, u of std 2, outlier channels, a sample 20 times smaller than the
others, a cotangent that is heavier in the last (ragged) row tile.  tests/test_tf_refs_cpu.py asserts that regime, and that no slice compared
here is smaller than 1e-3 of its tensor, for every case below — on a machine without a GPU.

References (tests/tf_refs.py, computed once per case and shared): X = float64 exact; R = float64 arithmetic between the roundings of the bf16
plan, one recipe per kernel family; F = the same arithmetic as X in float32.  H is the HIP result.

  bf16   max|H - X|_s <= 2 max|R - X|_s + 2e-5 max|X|_s  for every slice s;  ||H - X||_s <= 1.5 ||R - X||_s + 2e-5 ||X||_s  for s of >= 1024 elements
  fp32   max|H - X|_s <= 4 max|F - X|_s + 1e-6 max|X|_s

Slices: to_qkv.weight.grad by q / k / v rows and head; to_out weight by head columns; fc1 / fc2 weights and the fc1 bias by 64-wide block of
the hidden dimension; y and dx by row tile of the family's tile height (the ragged last one included) and by first / last row of every
sample; bias and LayerNorm vectors whole.  No bound is tuned to what the kernels give: the factors are those of EXPERIMENTS 5.12, the measured
ratios (error / bound, printed by every test) are tabulated in 5.13.  29 of the 10 900 slice checks exceed their bound for reasons that are not
in a kernel; they are listed one by one with their figures in KNOWN below.  The q / k gradients of the n = 1 case, exactly zero in X and R,
are held to an absolute f32 noise floor instead (tests/tf_cases.py::structural_zero)."""
import ctypes as C

import pytest
import torch

import tf_cases as K
import tf_refs as T

pytestmark = pytest.mark.gpu

from m3l_amd import Transformer  # noqa: E402
from m3l_amd import _lib as L  # noqa: E402

DEV = "cuda:0"
_SETTERS = {"attn_block": "m3l_set_attn_block", "t192": "m3l_set_t192", "t192_tt": "m3l_set_t192_tt", "enc_mega": "m3l_set_enc_mega",
            "rowln": "m3l_set_rowln", "residual_bf16": "m3l_set_residual_bf16", "drop_h": "m3l_set_drop_h"}
_MODULES = {}


def _module(case):
    """the m3l_amd.Transformer of a case with the case's parameters, on the device (shared by the tests of the case)"""
    k = K._input_key(case)
    if k not in _MODULES:
        P, _, _ = K.inputs_of(case)
        tf = Transformer(case.D, case.depth, case.heads, case.dim_head, case.mlp)
        tf.load_state_dict(P, strict=True)
        _MODULES[k] = tf.to(DEV)
    return _MODULES[k]


def _plan(case, tf):
    """the library's kernel selection for the case under the switches in force (m3l_transformer_plan: what forward and backward dispatch on)"""
    out = L.TfPlan()
    L.check(L.lib().m3l_transformer_plan(C.byref(tf._cfg()), case.B, case.n, None, C.byref(out)), "m3l_transformer_plan")
    return out


def _assert_family(case, sw, p):
    """With the case's switches in force the plan p selects the family the case is named after, for every half layer and both directions
    (no quiet fall-back to another one), and the row tiles have the case's height."""
    M, fam = case.B * case.n, case.family
    fields = {f: getattr(p, f) for f in ("fwd_attn", "fwd_outproj", "fwd_mlp", "bwd_mlp", "bwd_attn", "bwd_qkv")}
    block = p.fwd_attn == L.TF_BLOCK and p.fwd_outproj == L.TF_IN_BLOCK
    mlp_block = p.fwd_mlp == L.TF_BLOCK and p.bwd_mlp == L.TF_BLOCK
    tiles = bool({L.TF_T192, L.TF_TAIL_T192, L.TF_IN_TAIL} & set(fields.values()))
    if fam == "perop_dh":
        assert case.dim_head != 64 and p.per_op                  # every layer on the per-op chain
    if fam in ("perop", "perop_dh"):
        assert set(fields.values()) == {L.TF_PER_OP, L.TF_GEMM} and not p.rowln, fields
    elif fam == "rowln":
        assert p.rowln_cfg and p.rowln and not block and not tiles
        assert fields == dict(fwd_attn=L.TF_PER_OP, fwd_outproj=L.TF_ROWLN, fwd_mlp=L.TF_ROWLN, bwd_mlp=L.TF_ROWLN, bwd_attn=L.TF_PER_OP, bwd_qkv=L.TF_ROWLN)
    elif fam.startswith("block") or fam.startswith("mega"):
        assert block and mlp_block and not tiles, fields
        assert (p.bwd_attn == L.TF_BLOCK) == (p.bwd_qkv == L.TF_IN_BLOCK) == (fam != "block1")
        assert (p.mega_fwd, p.mega_bwd) == (sw["enc_mega"] & 1, sw["enc_mega"] >> 1 & 1)
    else:                                                # row tiles
        assert not block and p.fwd_mlp in (L.TF_T192, L.TF_IN_TAIL) and p.bwd_mlp == L.TF_T192 and p.bwd_qkv == L.TF_T192, fields
        assert p.row_tiles == -(-M // case.tile), (M, case.tile)
        assert (p.fwd_attn == L.TF_T192) == (p.bwd_attn == L.TF_T192) == (case.kt is None)


def _hip(case, dt, rb, drop_h=0, sw=None):
    """-> (tensors of the HIP run, whether the stack ran the bf16 residual stream, the plan of a bf16 run).  Every switch is restored whatever happens."""
    lib = L.lib()
    tf = _module(case)
    tf.compute_dtype = dt
    _, x, cot = K.inputs_of(case)
    x, cot = x.to(DEV), cot.to(DEV)
    want = list(dict(case.sw, **(sw or {})).items()) + [("residual_bf16", rb), ("drop_h", drop_h)]
    old = []
    try:
        for name, v in want:
            old.append((name, getattr(lib, _SETTERS[name])(v)))
        ran_rb = bool(lib.m3l_transformer_rb(C.byref(tf._cfg()), case.B, case.n)) if dt == "bf16" else False
        plan = _plan(case, tf) if dt == "bf16" else None
        if plan is not None:
            _assert_family(case, dict(case.sw, **(sw or {})), plan)
        tf.zero_grad(set_to_none=True)
        xg = x.clone().requires_grad_(True)
        y = tf(xg)
        (y * cot).sum().backward()
        torch.cuda.synchronize()
    finally:
        for name, v in reversed(old):
            getattr(lib, _SETTERS[name])(v)
    return T.tensors_of((y.detach().cpu(), xg.grad.cpu(), {k: p.grad.cpu().clone() for k, p in tf.named_parameters()})), ran_rb, plan


# Findings (EXPERIMENTS 5.13): the slices that exceed the issue's bound, each with (error, bound) as measured.  None has a cause in a kernel:
# H and R are two realisations of a rounding process that a 1e-6 relative change of the input decorrelates completely (the same recipe
# evaluated in float32 instead of float64 is as far from R as H is), so where R's own error in a slice happens to be small the factors 1.5 / 2
# are not enough.  The bounds stay as they are, and so does every slice: test_slices holds each listed slice to its recorded error (HELD),
# every other slice of the same run to the issue's bound, and test_known_slice_meets_the_issue_bound keeps asserting the issue's bound on the
# listed ones — expected to fail, strictly, so that a figure that moves either way is seen.  (The one-launch runs are bit-identical to each
# other, and the n = 200 row-tile runs share the per-op attention: hence the repeated figures.)
_QKV = "layers.%d.0.to_qkv.weight"
KNOWN = {
    ("perop-D192h3x64m768n40B3d2-bf16-rb0", _QKV % 1, "q head 1", "l2"): (3.776, 2.747),
    ("perop-D192h3x64m768n40B3d2-bf16-rb0", _QKV % 1, "q head 2", "l2"): (3.276, 3.241),
    ("perop-D192h3x64m768n40B3d2-bf16-rb0", _QKV % 1, "k head 1", "l2"): (4.051, 2.564),
    ("rowln-D192h3x64m768n40B3d2-bf16-rb0", _QKV % 1, "q head 1", "l2"): (3.788, 2.936),
    ("rowln-D192h3x64m768n40B3d2-bf16-rb0", _QKV % 1, "k head 1", "l2"): (4.069, 2.848),
    ("rowln-D192h3x64m768n40B3d2-bf16-rb1", _QKV % 1, "q head 1", "l2"): (3.788, 2.936),      # (the epilogue family never runs the bf16 residual stream)
    ("rowln-D192h3x64m768n40B3d2-bf16-rb1", _QKV % 1, "k head 1", "l2"): (4.069, 2.848),
    ("block1-D192h3x64m64n47B2d2-bf16-rb1", _QKV % 1, "q head 2", "l2"): (5.834, 5.774),
    ("block3-D192h3x64m64n47B2d2-bf16-rb1", _QKV % 1, "q head 2", "l2"): (5.834, 5.774),
    **{(f"mega{m}-D192h3x64m768n48B3d5-bf16-rb{rb}", _QKV % 4, f"{part} head 1", "l2"): fig
       for m, rb in ((1, 0), (2, 0), (2, 1), (3, 0), (3, 1))          # (bit 2 keeps the fp32 residual stream: rb1 = rb0 there)
       for part, fig in (("q", (3.193, 2.982)), ("k", (3.073, 3.019)))},
    **{(f"rowtile_tt{tt}-D192h3x64m384n200B2d2-bf16-rb1", name, label, kind): fig for tt in (12, 6)
       for name, label, kind, fig in (("dx", "sample 0 row 0", "max", (1.176, 1.095)), (_QKV % 0, "q head 1", "l2", (22.25, 20.86)),
                                      (_QKV % 0, "k head 1", "max", (7.105, 5.397)), (_QKV % 0, "k head 1", "l2", (22.61, 20.65)))},
    ("rowtile_tt12-D384h4x64m768n75B4d2-bf16-rb0", _QKV % 1, "k head 2", "l2"): (9.066, 8.806),
    # one bf16 step of an outlier channel of the residual stream (0.25 at |x| = 45) moves this row's final LayerNorm by 0.1
    ("rowtile_tt12-D384h4x64m768n75B4d2-bf16-rb1", "y", "sample 2 row 74", "max"): (0.1376, 0.06441),
}
# A listed slice may not exceed its recorded error by more than this.  The kernels' results and the float64 references reproduce bit for bit,
# so the recorded four digits are met as they stand; 10 % leaves room for another CPU's BLAS in R and none for a regression, which — the
# errors being sums of thousands of roundings — moves a slice by its own size or not at all.
HELD = 1.10
_RESULTS = {}


def _run_id(case, dt, rb):
    return f"{case.id}-{dt}-rb{rb}"


def _checked(case, dt, rb):
    """(worst ratios, failures, ran_rb) of a run, computed once"""
    rid = _run_id(case, dt, rb)
    if rid not in _RESULTS:
        got, ran_rb, _ = _hip(case, dt, rb)
        X = K.reference(case, "X")
        Y = K.reference(case, "R", ran_rb) if dt == "bf16" else K.reference(case, "F")
        assert set(got) == set(X)
        _RESULTS[rid] = K.check(case, got, X, Y, dt) + (ran_rb,)
    return _RESULTS[rid]


def _runs():
    return [pytest.param(c, dt, rb, id=_run_id(c, dt, rb)) for c in K.CASES for dt in c.dtypes for rb in ((0, 1) if dt == "bf16" else (0,))]


@pytest.mark.parametrize("case,dt,rb", _runs())
def test_slices(case, dt, rb):
    """every slice at the issue's bound, except the slices listed in KNOWN, which are held to their recorded error"""
    worst, fails, ran_rb = _checked(case, dt, rb)
    for kind in sorted(worst):
        r, name, label = worst[kind]
        print(f"\n[slices] {case.family} {case.id} {dt} rb{rb}/{int(ran_rb)} {kind} {r:.3f} {name} {label}", end="")
    rid = _run_id(case, dt, rb)
    new = [f for f in fails if (rid,) + f[:3] not in KNOWN]
    assert not new, (len(new), new[:8])
    moved = [f for f in fails if (rid,) + f[:3] in KNOWN and f[3] > HELD * KNOWN[(rid,) + f[:3]][0]]
    assert not moved, moved


_BY_ID = {_run_id(c, dt, rb): (c, dt, rb) for c in K.CASES for dt in c.dtypes for rb in (0, 1)}


@pytest.mark.parametrize("key", [pytest.param(k, id="-".join(k).replace(" ", "_"),
                                              marks=pytest.mark.xfail(strict=True, reason="finding, EXPERIMENTS 5.13: %.4g / %.4g = %.2f" % (v + (v[0] / v[1],))))
                                 for k, v in KNOWN.items()])
def test_known_slice_meets_the_issue_bound(key):
    """the issue's bound on each slice of KNOWN: not met, for the reason given there; the bound is not moved"""
    assert key[0] in _BY_ID, key
    _, fails, _ = _checked(*_BY_ID[key[0]])
    assert not [f for f in fails if f[:3] == key[1:]], key


MEGA = [c for c in K.CASES if c.family == "mega3" and c.depth in (2, 5)]


@pytest.mark.parametrize("rb", [0, 1])
@pytest.mark.parametrize("case", MEGA, ids=lambda c: c.id)
def test_one_launch_stack_is_bit_identical_on_these_inputs(case, rb):
    """enc_mega bits 1 / 2 / 3 against one launch per half layer (test_whole_stack_forward_launch_is_bit_identical, on peaked inputs; depth 5
    leaves a remainder group in the grouped backward)"""
    megas = (0, 1, 2, 3) if rb == 0 else (0, 1)          # (the grouped backward launch, bit 2, runs the fp32 residual stream only)
    res = {m: _hip(case, "bf16", rb, sw={"enc_mega": m})[0] for m in megas}
    for m in megas[1:]:
        for k in res[0]:
            assert torch.equal(res[0][k], res[m][k]), (m, k)


DROP_H = [c for c in K.CASES if c.depth == 2 and (c.family, c.n) in (("block3", 48), ("block3", 33), ("rowtile_tt12", 100), ("rowtile_tt6", 64))]


@pytest.mark.parametrize("rb", [0, 1])
@pytest.mark.parametrize("case", DROP_H, ids=lambda c: c.id)
def test_drop_h_is_bit_identical_on_these_inputs(case, rb):
    """m3l_set_drop_h(1): the fused feed-forward kernels do not save h, the fc2 weight gradient recomputes it from u — same bits
    (test_drop_h_is_bit_identical, on inputs whose u reaches both GELU tails)"""
    a, b = _hip(case, "bf16", rb, drop_h=0)[0], _hip(case, "bf16", rb, drop_h=1)[0]
    for k in a:
        assert torch.equal(a[k], b[k]), k


# one case per family, at the smallest depth the family has: (family, D, n, depth)
NAMED = [("perop", 192, 40, 1), ("perop_dh", 128, 33, 2), ("block1", 128, 17, 2), ("block3", 128, 17, 2), ("mega1", 192, 48, 2), ("mega2", 192, 48, 2),
         ("mega3", 192, 48, 2), ("rowtile_tt12", 192, 100, 1), ("rowtile_tt12", 256, 75, 2), ("rowln", 192, 40, 1)]
# the profiler kinds that belong to one family; ln_fwd, ln_bwd, gemm_nt..., wgrad..., prep_weights, cast, reduce_batch, colsum run under all
FAMILY_KINDS = {"enc_fwd_mega", "enc_bwd_mega", "attn_block_fwd", "attn_block_bwd", "mlp_block_fwd", "mlp_block_bwd", "attn_t192_fwd", "attn_t192_bwd",
                "attn_tail_mlp_t192_fwd", "mlp_t192_fwd", "mlp_t192_bwd", "qkv_bwd_t192", "gemm_nt_lnfwd", "gemm_nt_lnbwd", "attn_fwd", "attn_bwd"}


def _kinds_of(p):
    """the family kinds a forward + backward under plan p launches"""
    fwd = {"enc_fwd_mega"} if p.mega_fwd else {
        {L.TF_BLOCK: "attn_block_fwd", L.TF_T192: "attn_t192_fwd", L.TF_PER_OP: "attn_fwd"}[p.fwd_attn],
        {L.TF_ROWLN: "gemm_nt_lnfwd"}.get(p.fwd_outproj),
        {L.TF_IN_TAIL: "attn_tail_mlp_t192_fwd", L.TF_BLOCK: "mlp_block_fwd", L.TF_T192: "mlp_t192_fwd", L.TF_ROWLN: "gemm_nt_lnfwd"}.get(p.fwd_mlp)}
    bwd = {"enc_bwd_mega"} if p.mega_bwd else {
        {L.TF_BLOCK: "mlp_block_bwd", L.TF_T192: "mlp_t192_bwd", L.TF_ROWLN: "gemm_nt_lnbwd"}.get(p.bwd_mlp),
        {L.TF_BLOCK: "attn_block_bwd", L.TF_T192: "attn_t192_bwd", L.TF_PER_OP: "attn_bwd"}[p.bwd_attn],
        {L.TF_T192: "qkv_bwd_t192", L.TF_ROWLN: "gemm_nt_lnbwd"}.get(p.bwd_qkv)}
    return (fwd | bwd) - {None}


@pytest.mark.parametrize("key", NAMED, ids=lambda k: "%s-D%dn%dd%d" % k)
def test_plan_names_the_kernels_that_run(key):
    """forward + backward of one case per family under the profiler: the family kernels launched are EXACTLY those the plan names — what
    m3l_transformer_plan says and what the dispatcher does cannot drift apart"""
    case, = [c for c in K.CASES if (c.family, c.D, c.n, c.depth) == key]
    lib = L.lib()
    lib.m3l_prof_begin(None, 1)
    try:
        plan = _hip(case, "bf16", 1)[2]
    finally:
        lib.m3l_prof_end()
    ran = set()
    for i in range(lib.m3l_prof_count()):
        name = C.create_string_buffer(96)
        a, b, c_, d = C.c_double(), C.c_long(), C.c_double(), C.c_double()
        lib.m3l_prof_get(i, name, 96, C.byref(a), C.byref(b), C.byref(c_), C.byref(d))
        if b.value:
            ran.add(name.value.decode().split("[")[0])
    print(f"\n[plan] {case.id}: {sorted(ran)}", end="")
    assert ran & FAMILY_KINDS == _kinds_of(plan), (sorted(ran & FAMILY_KINDS), sorted(_kinds_of(plan)))
