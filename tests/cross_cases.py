"""What tests/cross_probe.hip is asked and what it should answer: the cases for k_cross_mfma<KS,4> and for the resident observation
stage (cross_stage<lds_cptr | glb_cptr>, cross_ks<2 | 8, lds_cptr, true> with the one-statement tile loop cross_loop_lds_2x2), the
request / result files, the build line, the references, and a plain restatement of which branch of the kernels each case takes.

The operands are small integers stored as doubles and NOT centred, so every product and every sum is exact in FP64 whatever the
order of summation, and the answer is held to the BITS of an int64 matrix product: an error that treats every observation alike --
the wrong y row, the wrong k lane, a k-step read twice, result rows stored to the wrong particles -- changes it, where on centred data
(sum_i x~_i = 0) it would change nothing a log-posterior can show.  One real-valued companion per kernel instance (standard normals,
np.longdouble reference) is held to the a-priori bound of recursive summation.

No GPU is needed to import or run anything here; tests/test_cross_host.py runs it on the CPU, tests/test_gpu_cross.py against the device."""
import os
import re
import struct
import zlib

import numpy as np

import device_math_cases as DM

ROOT, CSRC = DM.ROOT, DM.CSRC
PROBE_SRC = os.path.join(ROOT, "tests", "cross_probe.hip")

MAGIC = 0x3153524344434D44     # "DMCDCRS1"
SENTINEL = 0x7FF8DEAD0000BEEF  # what the probe pre-fills every output with: a quiet NaN no arithmetic produces
ld = np.longdouble
U = 2.0 ** -53
MAX_LDS = 150 * 1024           # kMaxDynLds (test_cross_host checks it against demc_constants.hpp)

KIND_CROSS, KIND_STAGE = 0, 1
FN_STAGE_LDS, FN_STAGE_GLB, FN_KS2_ASM, FN_KS8 = 0, 1, 2, 3
FN_NAME = {0: "cross_stage<lds_cptr>", 1: "cross_stage<glb_cptr>", 2: "cross_ks<2,lds_cptr,true>", 3: "cross_ks<8,lds_cptr,true>"}


# ---- the build line: csrc/Makefile's FLAGS, less -shared -fPIC (device_math_cases reads them) ------------------------------------
def probe_build_command(exe):
    cmd = DM.probe_build_command(exe)
    return [PROBE_SRC if a == DM.PROBE_SRC else a for a in cmd]


# ---- what the header says (a constant that moves shows up in test_cross_host's coverage test) ------------------------------------
def header_constants():
    txt = open(os.path.join(CSRC, "demc_kernels.hpp")).read()

    def ints(pattern):
        m = re.search(pattern, txt)
        assert m, "csrc/demc_kernels.hpp no longer says %r" % pattern
        return tuple(int(v) for v in m.groups())
    inst = re.search(r"#define DEMC_CROSS_INSTANCES\(X\)((?: X\(\d+, \d+\))+)", txt)
    assert inst, "DEMC_CROSS_INSTANCES not found"
    return dict(
        mtmax=ints(r"constexpr int MTMAX = KS >= (\d+) \? (\d+) : (\d+);"),  # (threshold, at or above it, below it)
        nq_shift=ints(r"int nq = \(n - 1\) >> (\d+);")[0],
        np_shift=ints(r"int np = \(r - 1\) >> (\d+);")[0],
        asm_at=ints(r"ASMLOOP && KS == (\d+) && MT == (\d+) &&"),
        instances=[(int(a), int(b)) for a, b in re.findall(r"X\((\d+), (\d+)\)", inst.group(1))])


# ---- which branch a case takes: the kernels' control flow, restated ----------------------------------------------------------------
def mt_ladder(KS, n_act, hc=None):
    """cross_ks: the cross_tiles<KS, MT> calls for n_act particles, as [(MT, padded)]; padded: MT = 4 over three tiles (rest == 3)"""
    thr, hi, lo = (hc or header_constants())["mtmax"]
    mtmax = hi if KS >= thr else lo
    n_pt, p0, calls = (n_act + 15) >> 4, 0, []
    while p0 + mtmax <= n_pt:
        calls.append((mtmax, False))
        p0 += mtmax
    rest = n_pt - p0
    if mtmax == 4 and rest == 3:
        calls.append((4, True))
    elif mtmax == 4 and rest == 2:
        calls.append((2, False))
    elif rest >= 1:
        calls.append((1, False))
    return calls


def ladder_name(calls):
    return "+".join("%d%s" % (mt if not pad else 3, "p" if pad else "") for mt, pad in calls)


def asm_trips(n, hc=None):
    """cross_loop_lds_2x2 on n >= 1 tiles: (four-tile trips, two-tile trips, 1 if the tail has two tiles)"""
    hc = hc or header_constants()
    nq = (n - 1) >> hc["nq_shift"]
    r = n - (1 << hc["nq_shift"]) * nq
    np_ = (r - 1) >> hc["np_shift"]
    return nq, np_, r - (1 << hc["np_shift"]) * np_ - 1


def takes_asm_loop(fn, KS, MT, hc=None):
    return fn == FN_KS2_ASM and (KS, MT) == (hc or header_constants())["asm_at"]


def chunk_tiles(n_tiles, n_chunks):
    """k_cross_mfma: observation tiles of every chunk"""
    per = (n_tiles + n_chunks - 1) // n_chunks
    return [max(0, min(c * per + per, n_tiles) - c * per) for c in range(n_chunks)]


def slots(c):
    """slot_of for q = 0 .. n_prop - 1"""
    q = np.arange(c["n_groups"] * c["n_act"])
    g = q // c["n_act"]
    pl = c["a_lo"] + q - g * c["n_act"]
    if c["glist"] is not None:
        g = np.asarray(c["glist"])[g]
    return g * c["Np"] + pl


# ---- operands ------------------------------------------------------------------------------------------------------------------------
def fragments(Xo, dpad):
    """demc_prep.hpp: Xf[tile][kstep][lane] = X[16 tile + (lane & 15)][4 kstep + (lane >> 4)]; Xo [16 tiles][dpad], padding included"""
    T = Xo.shape[0] // 16
    assert Xo.shape == (16 * T, dpad)
    return np.ascontiguousarray(Xo.reshape(T, 16, dpad // 4, 4).transpose(0, 2, 3, 1)).reshape(T, dpad // 4, 64)


def draw(rng, shape, real):
    return rng.standard_normal(shape) if real else rng.integers(-1023, 1024, shape).astype(np.float64)


def rng_of(name):
    return np.random.default_rng([20240611, zlib.crc32(name.encode())])


def cross_case(name, KS, d, N, n_chunks, mapping="main", real=False, nan_q=None):
    n_kpass = (d + 63) // 64 if d > 64 else 1
    dpad = 4 * KS * n_kpass
    assert d <= dpad
    if mapping == "main":
        geo = dict(n_groups=3, n_act=100, Np=201, a_lo=100, glist=[4, 0, 2], P=5 * 201)
    elif mapping == "one":
        geo = dict(n_groups=1, n_act=1, Np=3, a_lo=0, glist=None, P=3)
    else:
        geo = dict(n_groups=1, n_act=17, Np=19, a_lo=0, glist=None, P=19)
    rng = rng_of(name)
    c = dict(kind=KIND_CROSS, name=name, KS=KS, d=d, dpad=dpad, n_kpass=n_kpass, N=N, n_tiles=(N + 15) // 16, n_chunks=n_chunks, real=real,
             nan_q=nan_q, **geo)
    sl = slots(c)
    Y = np.full((c["P"], dpad), np.nan)  # a resting slot holds NaN: a row read from the wrong slot shows
    Y[sl] = draw(rng, (sl.size, dpad), real)
    if nan_q is not None:
        Y[sl[nan_q]] = np.nan
    Xo = np.zeros((16 * (c["n_tiles"] + 1), dpad))  # zero padded: the ragged tile, the dimensions past d, the all-zero tile behind the last
    Xo[:N, :d] = draw(rng, (N, d), real)
    c.update(Y=Y, Xo=Xo)
    return c


def stage_case(name, fn, dpad, wg, n_act, counts, xt_lo=0, real=False):
    nw = wg // 64
    assert len(counts) == nw and (fn == FN_STAGE_GLB or xt_lo == 0)
    rng = rng_of(name)
    # tiles as the source pointer sees them: NaN | wave 0's | NaN | wave 1's | NaN ... | NaN | the zero tile; in front, xt_lo tiles of NaN
    t_lo, t_hi, t = [0] * 8, [0] * 8, 1
    for w, n in enumerate(counts):
        t_lo[w], t_hi[w] = t, t + n
        t += n + 1
    zt, n_rel = t, t + 1
    Xo = np.full((16 * (xt_lo + n_rel), dpad), np.nan)
    for w in range(nw):
        r0, r1 = 16 * (xt_lo + t_lo[w]), 16 * (xt_lo + t_hi[w])
        Xo[r0:r1] = draw(rng, (r1 - r0, dpad), real)
    Xo[16 * (xt_lo + zt):] = 0.0
    nact_max = n_act + 3
    c = dict(kind=KIND_STAGE, name=name, fn=fn, KS=dpad // 4, dpad=dpad, wg=wg, n_act=n_act, nact_max=nact_max, n_src=xt_lo + n_rel, xt_lo=xt_lo,
             zt=zt, t_lo=t_lo, t_hi=t_hi, counts=list(counts), real=real, nan_q=None, Y=draw(rng, (n_act, dpad), real), Xo=Xo)
    assert lds_bytes(c) <= MAX_LDS, (name, lds_bytes(c))
    return c


def lds_bytes(c):
    nw = c["wg"] // 64
    tiles = 0 if c["fn"] == FN_STAGE_GLB else c["n_src"]
    return 8 * (c["n_act"] * c["dpad"] + ((nw * c["nact_max"] + 15) & ~15) + tiles * (c["dpad"] // 4) * 64)


# ---- the cases -------------------------------------------------------------------------------------------------------------------------
CROSS_KS = [(1, 4), (2, 8), (4, 16), (8, 32), (16, 64), (16, 100)]        # (KS, d): dpad = 4 KS, and d = 100 in two passes of 64
CROSS_OBS = [(1, 1), (17, 2), (33, 8), (1030, 8)]                         # (N, n_chunks)
NACT_LADDER = [1, 16, 17, 32, 33, 48, 64, 96, 100, 130]
NACT_KS16 = [16, 32, 48]
LONG_LIST = (512, (0, 1, 2, 3, 4, 5, 2, 1))                               # (threads, tiles of wave 0 .. 7)
SHORT_LIST = (256, (0, 1, 2, 3))                                          # KS >= 8: a tile is 4 or 8 KB of LDS
ASM_LISTS = dict(a=(512, (0, 1, 2, 3, 4, 5, 6, 7)), b=(512, (8, 9, 10, 11, 12, 13, 1, 4)))
ASM_NACT = [32, 96]
GLB_XT_LO = 3


def tile_list(KS):
    return SHORT_LIST if KS >= 8 else LONG_LIST


def cross_names():
    out = []
    for KS, d in CROSS_KS:
        for N, _ in CROSS_OBS:
            out.append("cross_ks%d_d%d_N%d_main" % (KS, d, N))
        out += ["cross_ks%d_d%d_N17_%s" % (KS, d, m) for m in ("one", "seventeen")]
    return out


def isolation_names():
    return ["cross_ks%d_d%d_isolation" % kd for kd in CROSS_KS]


def stage_names():
    out = []
    for src in ("lds", "glb"):
        for dpad in (4, 8, 16, 32, 64):
            out += ["stage_%s_d%d_n%d" % (src, dpad, n) for n in (NACT_KS16 if dpad == 64 else NACT_LADDER)]
    out += ["ks2asm_n%d" % n for n in NACT_LADDER] + ["ks8_n%d" % n for n in NACT_LADDER]
    return out


def asm_names():
    return ["asm_n%d_%s" % (n, k) for n in ASM_NACT for k in ASM_LISTS]


REAL_OF = {  # one real-valued companion per kernel instance: the integer case it shares its shape with
    **{"real_k_cross_mfma<%d,4>" % KS: "cross_ks%d_d%d_N1030_main" % (KS, d) for KS, d in CROSS_KS[:5]},
    "real_k_cross_mfma<16,4>_two_pass": "cross_ks16_d100_N1030_main",
    **{"real_cross_stage<%s_cptr>_d%d" % (src, dpad): "stage_%s_d%d_n%d" % (src, dpad, 48 if dpad == 64 else 100)
       for src in ("lds", "glb") for dpad in (4, 8, 16, 32, 64)},
    "real_cross_ks<2,lds_cptr,true>": "asm_n96_b",
    "real_cross_ks<8,lds_cptr,true>": "ks8_n100",
}


def make_case(name, real=False):
    m = re.fullmatch(r"cross_ks(\d+)_d(\d+)_N(\d+)_(main|one|seventeen)", name)
    if m:
        KS, d, N = (int(v) for v in m.groups()[:3])
        return cross_case(name if not real else "real:" + name, KS, d, N, dict(CROSS_OBS)[N], m.group(4), real)
    m = re.fullmatch(r"cross_ks(\d+)_d(\d+)_isolation", name)
    if m:  # every chunk of N = 1030 has tiles, so the NaN row reaches every plane
        return cross_case(name, int(m.group(1)), int(m.group(2)), 1030, 8, "main", nan_q=277)
    rname = name if not real else "real:" + name
    m = re.fullmatch(r"stage_(lds|glb)_d(\d+)_n(\d+)", name)
    if m:
        dpad, n_act = int(m.group(2)), int(m.group(3))
        wg, counts = tile_list(dpad // 4)
        glb = m.group(1) == "glb"
        return stage_case(rname, FN_STAGE_GLB if glb else FN_STAGE_LDS, dpad, wg, n_act, counts, GLB_XT_LO if glb else 0, real)
    m = re.fullmatch(r"ks2asm_n(\d+)", name)
    if m:
        return stage_case(rname, FN_KS2_ASM, 8, LONG_LIST[0], int(m.group(1)), LONG_LIST[1], 0, real)
    m = re.fullmatch(r"ks8_n(\d+)", name)
    if m:
        return stage_case(rname, FN_KS8, 32, SHORT_LIST[0], int(m.group(1)), SHORT_LIST[1], 0, real)
    m = re.fullmatch(r"asm_n(\d+)_(\w)", name)
    if m:
        wg, counts = ASM_LISTS[m.group(2)]
        return stage_case(rname, FN_KS2_ASM, 8, wg, int(m.group(1)), counts, 0, real)
    raise KeyError(name)


_cases = {}


def all_cases():
    """{name: case}, built once and shared (nothing changes a case)"""
    if not _cases:
        for n in cross_names() + isolation_names() + stage_names() + asm_names():
            _cases[n] = make_case(n)
        for n, of in REAL_OF.items():
            _cases[n] = make_case(of, real=True)
            _cases[n]["name"] = n
    return _cases


# ---- references ----------------------------------------------------------------------------------------------------------------------------
def planes(c):
    """every output plane (chunk plane of a k-pass, or wave) as (row0, row1 of Xo, col0, col1, T); T = tiles accumulated into its
    outputs, the zero tile that absorbs the odd end of the two-tile ping-pong included (the asm loop reads none)"""
    out = []
    if c["kind"] == KIND_CROSS:
        per = (c["n_tiles"] + c["n_chunks"] - 1) // c["n_chunks"]
        for kp in range(c["n_kpass"]):
            for ch, n in enumerate(chunk_tiles(c["n_tiles"], c["n_chunks"])):
                out.append((16 * ch * per if n else 0, 16 * (ch * per + n) if n else 0, 4 * c["KS"] * kp, 4 * c["KS"] * (kp + 1), n + (n & 1)))
    else:
        # (where some particle tiles take the asm loop and others the builtin loop, the larger count bounds both)
        all_asm = all(takes_asm_loop(c["fn"], c["KS"], mt) for mt, _ in mt_ladder(c["KS"], c["n_act"]))
        for w in range(c["wg"] // 64):
            n = c["t_hi"][w] - c["t_lo"][w]
            out.append((16 * (c["xt_lo"] + c["t_lo"][w]), 16 * (c["xt_lo"] + c["t_hi"][w]), 0, c["dpad"], n if all_asm else n + (n & 1)))
    return out


def y_rows(c, Y=None):
    """the y row of every q, the NaN row of an isolation case as zeros"""
    Y = c["Y"] if Y is None else Y
    Yq = (Y[slots(c)] if c["kind"] == KIND_CROSS else Y).copy()
    if c["nan_q"] is not None:
        Yq[c["nan_q"]] = 0.0
    return Yq


def out_index(c):
    """[plane][q] -> position in the output the probe returns"""
    n_pl = len(planes(c))
    if c["kind"] == KIND_CROSS:
        return np.arange(n_pl)[:, None] * c["P"] + slots(c)[None, :]
    return np.arange(n_pl)[:, None] * c["nact_max"] + np.arange(c["n_act"])[None, :]


def n_out(c):
    return len(planes(c)) * (c["P"] if c["kind"] == KIND_CROSS else c["nact_max"])


def reference_int(c, Y=None, Xo=None):
    """[plane][q] int64: Y.astype(int64) @ X.T.astype(int64), summed over the plane's observations"""
    assert not c["real"]
    Yq, Xo = y_rows(c, Y).astype(np.int64), (c["Xo"] if Xo is None else Xo)
    ref = np.zeros((len(planes(c)), Yq.shape[0]), np.int64)
    for i, (r0, r1, c0, c1, _) in enumerate(planes(c)):
        if r1 > r0:
            ref[i] = (Yq[:, c0:c1] @ Xo[r0:r1, c0:c1].astype(np.int64).T).sum(1)
    return ref


def magnitude(c):
    """[plane][q] sum_i sum_k |y_k x_ik| (float64: a bound's scale, and below 2^53 the integer cases' own exactness condition)"""
    Yq = np.abs(y_rows(c))
    return np.stack([Yq[:, c0:c1] @ np.abs(c["Xo"][r0:r1, c0:c1]).sum(0) for r0, r1, c0, c1, _ in planes(c)])


def reference_ld(c):
    """[plane][q] np.longdouble: every product rounded once to 64 bits, then numpy's pairwise sum"""
    Yq, Xo = y_rows(c).astype(ld), c["Xo"].astype(ld)
    ref = np.zeros((len(planes(c)), Yq.shape[0]), ld)
    for i, (r0, r1, c0, c1, _) in enumerate(planes(c)):
        if r1 > r0:
            x = np.ascontiguousarray(Xo[r0:r1, c0:c1]).ravel()
            for q in range(Yq.shape[0]):
                ref[i, q] = (np.tile(Yq[q, c0:c1], r1 - r0) * x).sum()
    return ref


def real_bound(c):
    """(4 KS T + 6) 2^-53 sum |y x|: recursive summation of the 4 KS T products accumulated into an output, plus the fold of the
    sixteen columns (four additions) with room for the two ends"""
    T = np.array([p[4] for p in planes(c)], np.float64)
    return (4 * c["KS"] * T + 6)[:, None] * U * magnitude(c)


# ---- mutations of the operands that a layout error is equivalent to (test_cross_host: each must change the reference) --------------
def swap_k_lanes(c, j1, j2):
    """Y with the k lanes j1 and j2 of every k-step exchanged (the A fragment's lane >> 4)"""
    Y = c["Y"].copy()
    a, b = np.arange(j1, c["dpad"], 4), np.arange(j2, c["dpad"], 4)
    Y[:, a], Y[:, b] = c["Y"][:, b], c["Y"][:, a]
    return Y


def kstep1_from_kstep0(c):
    """Xo with k-step 1 of every pass replaced by its k-step 0 (the asm loop's offset:512 read as offset:0)"""
    Xo = c["Xo"].copy()
    for k0 in range(0, c["dpad"], 4 * c["KS"]):
        Xo[:, k0 + 4:k0 + 8] = c["Xo"][:, k0:k0 + 4]
    return Xo


def units(c):
    """the (plane, 16-row fragment) pairs that hold sums of at least one tile, as (plane, q0, q1): what one MFMA accumulator answers for"""
    nq = y_rows(c).shape[0]
    return [(i, q0, min(q0 + 16, nq)) for i, p in enumerate(planes(c)) if p[1] > p[0] for q0 in range(0, nq, 16)]


# ---- request / result files ------------------------------------------------------------------------------------------------------------
def header(c):
    h = [0] * 32
    Xf = fragments(c["Xo"], c["dpad"])
    h[0], h[1], h[2], h[3] = c["kind"], c["Y"].size, Xf.size, n_out(c)
    if c["kind"] == KIND_CROSS:
        gl = c["glist"] or []
        h[4:15] = [c["KS"], c["dpad"], c["n_kpass"], c["n_tiles"], c["n_chunks"], c["n_groups"], c["n_act"], c["Np"], c["a_lo"], c["P"], len(gl)]
        h[15:15 + len(gl)] = gl
    else:
        h[4:12] = [c["fn"], c["dpad"], c["wg"], c["n_act"], c["nact_max"], c["n_src"], c["xt_lo"], c["zt"]]
        h[12:20], h[20:28] = c["t_lo"], c["t_hi"]
    return h, Xf


def write_request(path, cases):
    with open(path, "wb") as f:
        f.write(struct.pack("<QQ", MAGIC, len(cases)))
        for c in cases:
            h, Xf = header(c)
            f.write(struct.pack("<32q", *h))
            f.write(np.ascontiguousarray(c["Y"], np.float64).tobytes())
            f.write(Xf.tobytes())


def read_request(path):
    """[(hdr[32], Y flat, Xf flat)]"""
    buf = open(path, "rb").read()
    magic, nc = struct.unpack_from("<QQ", buf, 0)
    assert magic == MAGIC
    off, out = 16, []
    for _ in range(nc):
        h = list(struct.unpack_from("<32q", buf, off))
        off += 256
        Y = np.frombuffer(buf, np.float64, h[1], off).copy()
        off += 8 * h[1]
        X = np.frombuffer(buf, np.float64, h[2], off).copy()
        off += 8 * h[2]
        out.append((h, Y, X))
    assert off == len(buf)
    return out


def write_result(path, outs):
    """outs: [(kind, out flat)]"""
    with open(path, "wb") as f:
        f.write(struct.pack("<QQ", MAGIC, len(outs)))
        for kind, o in outs:
            o = np.ascontiguousarray(o, np.float64)
            f.write(struct.pack("<qq", kind, o.size))
            f.write(o.tobytes())


def read_result(path):
    buf = open(path, "rb").read()
    magic, nc = struct.unpack_from("<QQ", buf, 0)
    assert magic == MAGIC
    off, outs = 16, []
    for _ in range(nc):
        kind, n = struct.unpack_from("<qq", buf, off)
        off += 16
        outs.append((kind, np.frombuffer(buf, np.float64, n, off).copy()))
        off += 8 * n
    assert off == len(buf), "the result file is longer or shorter than its headers say"
    return outs


def stand_in(c):
    """what a correct probe returns, formed on the host in float64 from the fragment-ordered request (it checks the files, the
    fragment order and the references, not the kernels)"""
    h, Xf = header(c)
    dpad = c["dpad"]
    Xo = Xf.reshape(-1, dpad // 4, 4, 16).transpose(0, 3, 1, 2).reshape(-1, dpad)  # the inverse of fragments()
    out = np.full(n_out(c), np.nan)
    out.view(np.uint64)[:] = SENTINEL
    Yq = c["Y"][slots(c)] if c["kind"] == KIND_CROSS else c["Y"]
    idx = out_index(c)
    for i, (r0, r1, c0, c1, _) in enumerate(planes(c)):
        out[idx[i]] = (Yq[:, c0:c1] @ Xo[r0:r1, c0:c1].T).sum(1) if r1 > r0 else 0.0
    return out
