"""The matrix-core cross term S_p = sum_i y_p . x_i of STREAMING mode, run as DEVICE code on operands that make the comparison exact:
k_cross_mfma<KS,4> (KS = 1 .. 16, one and two k-passes) launched as launch_loglike launches it, and the resident observation stage --
cross_stage<lds_cptr | glb_cptr> and cross_ks<2 | 8, lds_cptr, true> with the one-statement tile loop cross_loop_lds_2x2 -- called as
k_propose<..., STREAM> and k_res_mvn<..., true, DT> call it.

Every other test that reaches these kernels sees their sum only through a log-posterior of CENTRED data, where sum_i x~_i = 0 and the
cross term is zero up to rounding whatever y row, k lane or result row the kernel takes.  Here Y and X are integers of [-1023, 1023]
stored as doubles and not centred: every sum is exact in FP64 in any order, and the answer is held to the bits of
Y.astype(int64) @ X.T.astype(int64).  Resting slots of Ypad, tiles outside a wave's range (the zero tile excepted) hold NaN; every
output is pre-filled with a NaN of known bits, which every entry the case does not address must keep.

tests/cross_probe.hip includes the kernels' own header and is compiled with the FLAGS line of csrc/Makefile (less -shared -fPIC).  The
module builds the probe and runs it ONCE, in a child process, on every case (tests/cross_cases.py holds them and the references); each
test only reads the answers.  A failed build, a non-zero exit or a timeout fails every test from the kept message and nothing is
started on the GPU again."""
import subprocess

import numpy as np
import pytest

import cross_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("cross")
    exe, req, res = (str(d / n) for n in ("cross_probe", "request.bin", "result.bin"))
    cases = C.all_cases()
    state = dict(cases=cases, out={}, error=None)
    try:
        b = subprocess.run(C.probe_build_command(exe), capture_output=True, text=True, timeout=600)
        if b.returncode != 0:
            state["error"] = "the probe did not build:\n" + b.stderr[-4000:]
            return state
        C.write_request(req, list(cases.values()))
        r = subprocess.run([exe, req, res], capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            state["error"] = "the probe ended with status %d:\n%s%s" % (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
            return state
        state["error"] = load_answers(state, res)
    except subprocess.TimeoutExpired as e:
        state["error"] = "timed out: %r" % (e.cmd,)
    return state


def load_answers(state, res):
    """fills state["out"] from a result file; the error message, or None"""
    outs, cases = C.read_result(res), state["cases"]
    if [(k, o.size) for k, o in outs] != [(c["kind"], C.n_out(c)) for c in cases.values()]:
        return "the result file does not answer the request case by case"
    state["out"] = {name: o for name, (_, o) in zip(cases, outs)}
    return None


def answers(probe, name):
    if probe["error"]:
        pytest.fail(probe["error"])
    return probe["cases"][name], probe["out"][name]


def bits(v):
    return np.ascontiguousarray(v, np.float64).view(np.uint64)


def check_exact(c, out):
    """every addressed entry has the bits of the integer reference (an empty plane: +0.0, a NaN row: NaN in every plane), every
    other entry the bits it was pre-filled with"""
    ref, idx = C.reference_int(c), C.out_index(c)
    want = ref.astype(np.float64)
    assert (want.astype(np.int64) == ref).all()  # (below 2^53)
    got = out[idx]
    rows = np.ones(ref.shape[1], bool)
    if c["nan_q"] is not None:
        rows[c["nan_q"]] = False
        assert all(p[1] > p[0] for p in C.planes(c))
        assert np.isnan(got[:, c["nan_q"]]).all(), "the NaN row did not reach every plane of its particle"
    bad = np.argwhere(bits(got[:, rows]) != bits(want[:, rows]))
    assert bad.size == 0, "%s: %d of %d sums differ, first (plane, q) %r: got %r, exact %r" % (
        c["name"], len(bad), want[:, rows].size, tuple(bad[0]), got[:, rows][tuple(bad[0])], want[:, rows][tuple(bad[0])])
    rest = np.ones(out.size, bool)
    rest[idx.ravel()] = False
    assert rest.sum() == out.size - idx.size and (bits(out[rest]) == C.SENTINEL).all(), "%s: an entry the case does not address was written" % c["name"]


@pytest.mark.parametrize("name", C.cross_names())
def test_cross_mfma_is_the_exact_product(probe, name):
    """k_cross_mfma<KS,4>, KS = 1, 2, 4, 8, 16 at dpad = 4 KS and KS = 16 at dpad = 128 (d = 100) in two passes (k0 = 0 / 64, part0 = 0 /
    n_chunks, every plane held to its own half of the dimensions), grid n_ptiles * n_chunks of 256 threads.  Slots: three launch groups
    glist = {4, 0, 2} of five, n_act = 100 from a_lo = 100 of Np = 201 (n_prop = 300: two particle tiles, the second with 44 proposals
    -- two full 16-row fragments and one of 12), n_prop = 1, and n_prop = 17 without a glist.  Observations: N = 1, 17 (two tiles, one
    ragged), 33 in 8 chunks (chunks 3 .. 7 are empty and store +0.0) and 1030 in 8 chunks (65 tiles, 9 a chunk, the last chunk 2: odd
    and even trip counts of the ping-pong).  Resting slots and the planes' resting entries keep the pre-filled bits."""
    check_exact(*answers(probe, name))


def test_cross_mfma_two_passes_add_up_to_the_whole(probe):
    """d = 100 > 64: the planes of the two passes, added, are the product over all 100 dimensions"""
    c, out = answers(probe, "cross_ks16_d100_N1030_main")
    got = out[C.out_index(c)].reshape(2, c["n_chunks"], -1).sum((0, 1))
    Yq, X = C.y_rows(c).astype(np.int64), c["Xo"].astype(np.int64)
    assert c["n_kpass"] == 2 and (got == (Yq @ X.T).sum(1)).all()


@pytest.mark.parametrize("name", C.isolation_names())
def test_cross_mfma_nan_row_stays_in_its_particle(probe, name):
    """one y row NaN: exactly that particle's outputs are NaN, in every chunk plane; every other output keeps its exact bits"""
    check_exact(*answers(probe, name))


@pytest.mark.parametrize("name", C.stage_names())
def test_resident_stage_is_the_exact_product(probe, name):
    """cross_stage<lds_cptr> and <glb_cptr> at dpad 4 .. 64, cross_ks<2,lds_cptr,true> and <8,lds_cptr,true>: one workgroup, every wave its
    own tile range [t_lo, t_hi) with t_lo != 0 of 0 .. 5 tiles (KS >= 8: 0 .. 3), the zero tile appended to the LDS copy or at
    n_tiles - xt_lo of a global source that starts at tile xt_lo = 3; n_act over the MT ladder (1, 2, 4, the rest == 3 padded tile,
    4 + 2, 4 + 3, 4 + 4 + 1; KS = 16: 1, 2, 2 + 1).  Every tile outside the waves' ranges but the zero tile is NaN; out[q >= n_act]
    keeps the pre-filled bits; a wave without tiles stores +0.0."""
    check_exact(*answers(probe, name))


@pytest.mark.parametrize("name", C.asm_names())
def test_asm_tile_loop_is_the_exact_product(probe, name):
    """cross_loop_lds_2x2 through cross_ks<2,lds_cptr,true> at n_act = 32 and 96 (MT = 2, and MT = 4 + 2): every n = 1 .. 13 tiles from
    t_lo != 0 -- four-tile trips 0 .. 3, two-tile trips 0 and 1, both tails -- and n = 0, where the statement is skipped and +0.0 is stored"""
    c, out = answers(probe, name)
    assert c["counts"] in ([0, 1, 2, 3, 4, 5, 6, 7], [8, 9, 10, 11, 12, 13, 1, 4])
    check_exact(c, out)


@pytest.mark.parametrize("name", list(C.REAL_OF))
def test_real_valued_companion(probe, name):
    """standard normals against an np.longdouble dot product: |error| <= (4 KS T + 6) 2^-53 sum_i sum_k |y_k x_ik|, T the tiles
    accumulated into the output (the zero tile included) -- the bound of recursive summation plus the fold, a priori.
    Measured on an MI355X: largest ratio to the bar 0.060 (cross_stage<glb_cptr> at dpad 4; DESIGN 8 has every instance's)."""
    c, out = answers(probe, name)
    ref, bar, idx = C.reference_ld(c), C.real_bound(c), C.out_index(c)
    err = np.abs(out[idx].astype(C.ld) - ref).astype(np.float64)
    live = bar > 0
    ratio = float((err[live] / bar[live]).max())
    print("%s: largest |error| / bar = %.3g (largest |error| %.3g)" % (name, ratio, err.max()))
    assert np.isfinite(out[idx]).all() and (err[~live] == 0).all()
    assert (err <= bar).all()
    rest = np.ones(out.size, bool)
    rest[idx.ravel()] = False
    assert (bits(out[rest]) == C.SENTINEL).all()
