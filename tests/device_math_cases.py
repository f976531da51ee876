"""What tests/device_math_probe.hip is asked and what it should answer: the arguments of every case (random points, every rounding
tie of the magic-number roundings with both neighbours, the clamps and the specials), the request / result files, a numpy stand-in
for the probe (libm forms: it checks the files and the references, not the kernels), and the high-precision references -- mpmath
at 40 digits for Phi, phi, log Phi, the LBA and the priors, np.longdouble for exp, softplus and 1/x.  No GPU is needed to import or
run anything here; tests/test_device_math_host.py runs it on the CPU, tests/test_gpu_device_math.py against the device."""
import os
import re
import shlex
import struct

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "differentialevolutionmcmc.jl_amd", "csrc")
PROBE_SRC = os.path.join(ROOT, "tests", "device_math_probe.hip")

MAGIC = 0x314D564544434D44
FN = dict(exp_nonpos=0, softplus_fast=1, softplus_tab=2, recip_pos=3, phi_table=4, log_phi_neg=5, lba2=6, lba3=7, lba_rt4=8,
          prior_term=9, box_muller=10)
YCOLS = {0: 0, 1: 0, 2: 0, 3: 0, 4: 0, 5: 0, 6: 8, 7: 8, 8: 8, 9: 3, 10: 1}
LBA_NA = dict(lba2=2, lba3=3, lba_rt4=4)

ld = np.longdouble
NAN, INF = float("nan"), float("inf")
PHI_S, PHI_HALF = 32.0, 272.0  # kPhiPerUnit, 8.5 kPhiPerUnit (test_device_math_host checks them against the header)


# ---- the build line: csrc/Makefile's FLAGS, less -shared -fPIC ------------------------------------------------------------------
def probe_build_command(exe):
    mk = open(os.path.join(CSRC, "Makefile")).read()
    var = {k: v.strip() for k, v in re.findall(r"^(HIPCC|ARCH) \?= (.+)$", mk, re.M)}
    flags = re.search(r"^FLAGS = (.+)$", mk, re.M).group(1).replace("$(ARCH)", var["ARCH"])
    flags = [f for f in shlex.split(flags) if f not in ("-shared", "-fPIC")]
    hipcc = os.environ.get("HIPCC", var["HIPCC"])
    return [hipcc] + flags + ["-I" + CSRC, PROBE_SRC, "-o", exe]


# ---- request / result files -----------------------------------------------------------------------------------------------------
def write_request(path, cases):
    """cases: [(fn, x[n], y[n_ycols, n] or None)]"""
    with open(path, "wb") as f:
        f.write(struct.pack("<QQ", MAGIC, len(cases)))
        for fn, x, y in cases:
            x = np.ascontiguousarray(x, np.float64)
            ny = YCOLS[fn]
            y = np.zeros((0, x.size)) if y is None else np.ascontiguousarray(y, np.float64)
            assert x.ndim == 1 and y.shape == (ny, x.size), (fn, x.shape, y.shape)
            f.write(struct.pack("<qqq", fn, x.size, ny))
            f.write(x.tobytes())
            f.write(y.tobytes())


def read_request(path):
    buf = open(path, "rb").read()
    magic, nc = struct.unpack_from("<QQ", buf, 0)
    assert magic == MAGIC
    off, cases = 16, []
    for _ in range(nc):
        fn, n, ny = struct.unpack_from("<qqq", buf, off)
        off += 24
        a = np.frombuffer(buf, np.float64, (1 + ny) * n, off).reshape(1 + ny, n)
        off += 8 * (1 + ny) * n
        cases.append((fn, a[0].copy(), a[1:].copy()))
    assert off == len(buf)
    return cases


def write_result(path, outs):
    """outs: [(fn, out[2, n])]"""
    with open(path, "wb") as f:
        f.write(struct.pack("<QQ", MAGIC, len(outs)))
        for fn, o in outs:
            o = np.ascontiguousarray(o, np.float64)
            assert o.ndim == 2 and o.shape[0] == 2
            f.write(struct.pack("<qq", fn, o.shape[1]))
            f.write(o.tobytes())


def read_result(path):
    buf = open(path, "rb").read()
    magic, nc = struct.unpack_from("<QQ", buf, 0)
    assert magic == MAGIC
    off, outs = 16, []
    for _ in range(nc):
        fn, n = struct.unpack_from("<qq", buf, off)
        off += 16
        outs.append((fn, np.frombuffer(buf, np.float64, 2 * n, off).reshape(2, n).copy()))
        off += 16 * n
    assert off == len(buf), "the result file is longer or shorter than its headers say"
    return outs


# ---- arguments ------------------------------------------------------------------------------------------------------------------
def with_neighbours(v):
    """every v with the double below and the double above it: [v0-, v0, v0+, v1-, ...]"""
    v = np.asarray(v, np.float64)
    return np.stack([np.nextafter(v, -INF), v, np.nextafter(v, INF)], 1).ravel()


def pack(parts):
    """{name: array} -> (the arrays in one, {name: slice})"""
    x, where, off = [], {}, 0
    for k, v in parts.items():
        v = np.asarray(v, np.float64)
        x.append(v)
        where[k] = slice(off, off + v.size)
        off += v.size
    return np.concatenate(x), where


def softplus_header():
    txt = open(os.path.join(CSRC, "demc_softplus_table.hpp")).read()
    return {k: float.fromhex(v) for k, v in re.findall(r"constexpr double (kSp\w+) = (-?0x[0-9a-fA-F.]+p[+-]?\d+);", txt)}


def header_ints(name):
    return {k: int(v) for k, v in re.findall(r"constexpr int (k\w+) = (-?\d+);", open(os.path.join(CSRC, name)).read())}


def exp_nonpos_args():
    ln2 = np.log(ld(2))
    n = np.arange(0, -1011, -1).astype(ld)
    ties = np.concatenate([(n - ld(0.5)) * ln2, (n + ld(0.5)) * ln2]).astype(np.float64)
    ties = ties[ties <= 0]  # (exp_nonpos is for a <= 0: (0 + 1/2) ln 2 is not an argument)
    return pack(dict(random=np.random.default_rng(11).uniform(-700.0, 0.0, 200000), ties=with_neighbours(ties),
                     specials=[0.0, -0.0, -5e-324, -700.0, -700.0000001, -1e300, -INF], nan=[NAN]))


def softplus_args():
    rng = np.random.default_rng(3)  # the point set of test_tables.test_softplus_table_of_the_row_streaming_kernel
    table_test = np.concatenate([rng.uniform(-40, 40, 300000), rng.uniform(-1, 1, 50000), rng.uniform(-690, -30, 20000),
                                 rng.uniform(30, 700, 20000), np.linspace(-0.01, 0.01, 2001), [0.0, -0.0, 700.0, -690.0]])
    c = ld(softplus_header()["kSpC"])
    k = np.arange(-int(np.floor(40 * float(c))), 0).astype(ld)  # the k of a in [-40, 0): a = (k + 1/2) / kSpC < 0
    k_ties = with_neighbours(((k + ld(0.5)) / c).astype(np.float64))
    j = np.arange(128).astype(ld)
    j_ties = with_neighbours(np.log((j + ld(0.5)) / ld(128)).astype(np.float64))  # exp(a) = (j + 1/2) / 128
    return pack(dict(table_test=table_test, k_ties=np.concatenate([k_ties, -k_ties]), j_ties=np.concatenate([j_ties, -j_ties]),
                     specials=[0.0, -0.0, 700.0, -700.0, 745.0, 1e300], below_clamp=[-745.0, -745.0000001, -1e300, -INF],
                     inf=[INF], nan=[NAN]))


def recip_pos_args():
    rng = np.random.default_rng(12)
    return pack(dict(random=np.exp(rng.uniform(np.log(1e-300), np.log(1e300), 200000)), pow2=2.0 ** np.arange(-996, 997),
                     one=with_neighbours([1.0]), decision_times=np.concatenate([rng.uniform(1e-3, 60.0, 20000), np.linspace(1e-3, 60.0, 2001)]),
                     denormal=[5e-324, 1e-310, 2.225073858507201e-308]))


def phi_table_args():
    """arguments zs = S z"""
    grid = np.linspace(-8.5, 8.5, 400001) * PHI_S  # the grid of test_tables.test_phi_table_of_the_lba_kernels
    ties = np.arange(int(2 * PHI_HALF)) + 0.5 - PHI_HALF
    return pack(dict(grid=grid, ties=with_neighbours(ties), ends=with_neighbours([-PHI_HALF, PHI_HALF]),
                     beyond=[-30.0 * PHI_S, 30.0 * PHI_S, -1e300, 1e300, -INF, INF], nan=[NAN]))


def log_phi_neg_args():
    table_test = np.concatenate([np.linspace(-8.5, 38.5, 4001), np.random.default_rng(4).uniform(-8.5, 38.5, 4000)])
    ties = (np.arange(376) + 0.5 - 68.0) / 8.0
    lo, hi = np.nextafter(-8.5, -INF), np.nextafter(38.5, INF)
    return pack(dict(table_test=table_test, ties=with_neighbours(ties), clamps=[-8.5, np.nextafter(-8.5, INF), np.nextafter(38.5, -INF), 38.5],
                     below=[lo, -9.0, -30.0, -1e300, -INF], far=np.geomspace(hi, 1e3, 2000), far_special=[1e150, 1e300, INF], nan=[NAN]))


LBA_TAIL_DRIFTS = ((3.0, 2.0, 1.0, 0.5), (-1.0, -2.0, 0.5, 1.0), (-3.0, -0.5, -1.0, -2.0), (12.0, -12.0, 9.0, 0.1))
LBA_ROWS = dict(lba3=7000, lba2=7000, lba_rt4=6000)  # 2e4 rows drawn like make_problem("lba") between the three instances


def lba_args(name):
    """x = rt, y = (choice, nu[0..3], A, k, tau): rows drawn like conftest.make_problem("lba"), the tails, and the trials whose
    factor is 0 (decision time not after tau, NaN)"""
    na, n = LBA_NA[name], LBA_ROWS[name]
    rng = np.random.default_rng(20 + na)
    y = np.zeros((8, n))
    y[0] = rng.integers(1, na + 1, n)
    y[1:1 + na] = rng.uniform(0.5, 4.0, (na, n))
    y[5], y[6], y[7] = rng.uniform(0.5, 1.1, n), rng.uniform(0.05, 0.4, n), rng.uniform(0.05, 0.45 * 0.9, n)
    rt = rng.uniform(0.45, 1.6, n)
    tail = [(0.25 + t, c, *d[:na], *(0.0,) * (4 - na), A, k, 0.25)
            for t in (1e-3, 5.0, 60.0) for A in (1e-3, 5.0) for k in (0.05, 0.4) for d in LBA_TAIL_DRIFTS for c in range(1, na + 1)]
    dead = [(r, 1, *(3.0, 2.0, 1.0, 0.5)[:na], *(0.0,) * (4 - na), 0.8, 0.2, tau)
            for r, tau in ((0.25, 0.25), (0.15, 0.25), (NAN, 0.25), (1e-300, 0.0), (1e-310, 0.0))]
    rows = np.array(tail + dead).T
    x, where = pack(dict(random=rt, tail=rows[0, :len(tail)], dead=rows[0, len(tail):]))
    return x, np.concatenate([y, rows[1:]], 1), where


PRIOR_KINDS = (1, 2, 3, 4, 6, 7, 8, 9)
PRIOR_PARAMS = {  # (a, b) as demc_set_priors takes them
    1: ((0.0, 1.0), (1.5, 0.2), (-3.0, 10.0), (0.8, 0.2)),                    # Normal(mean, sd)
    2: ((0.0, 1.0), (0.0, 0.1), (0.0, 25.0), (0.5, 2.0)),                     # Cauchy(a, b) truncated to [0, Inf)
    3: ((0.0, 1.0), (-2.0, 3.0), (0.0, 0.45), (-5.0, 1e300)),                 # Uniform(a, b)
    4: ((0.5, 0.5), (1.0, 1.0), (2.0, 5.0), (1.0, 3.0), (0.5, 1.0)),          # Beta(a, b)
    6: ((0.5, 1.0), (1.0, 2.0), (3.0, 0.5), (9.0, 0.1)),                      # Gamma(shape, scale)
    7: ((0.0, 1.0), (0.0, 0.2), (0.0, 30.0), (0.0, 1e-3)),                    # Exponential(scale b)
    8: ((0.0, 1.0), (-1.0, 0.5), (2.0, 2.0), (0.5, 1.0)),                     # LogNormal(mu, sigma)
    9: ((0.0, 1.0), (-3.0, 0.1), (2.0, 25.0), (0.0, 1e3)),                    # Cauchy(a, b)
}
PRIOR_PER_KIND = 200


def prior_support(kind, a, b):
    return {1: (-INF, INF), 2: (0.0, INF), 3: (a, b), 4: (0.0, 1.0), 6: (0.0, INF), 7: (0.0, INF), 8: (0.0, INF), 9: (-INF, INF)}[kind]


def prior_args():
    """x and y = (kind, a, b), PRIOR_PER_KIND rows per kind: for every parameter set both ends of the support with their
    neighbours (0 with its neighbours where the support is the line), +-1e-300, +-1e300, and interior points for the rest"""
    rng = np.random.default_rng(13)
    xs, ys = [], []
    for kind in PRIOR_KINDS:
        sets = PRIOR_PARAMS[kind]
        per = PRIOR_PER_KIND // len(sets)
        for a, b in sets:
            lo, hi = prior_support(kind, a, b)
            edge = list(with_neighbours([lo if np.isfinite(lo) else 0.0])) + (list(with_neighbours([hi])) if np.isfinite(hi) else [])
            edge += [1e-300, -1e-300, 1e300, -1e300]
            m = per - len(edge)
            u = rng.uniform(0, 1, m)
            if kind == 1:
                inner = a + b * (12 * u - 6)
            elif kind == 2:
                inner = b * np.exp(np.log(1e-3) + u * np.log(1e6))
            elif kind == 3:
                inner = lo + (min(hi, lo + 10.0) - lo) * u
            elif kind == 4:
                inner = np.concatenate([[1e-10, 1 - 1e-10], u[2:]])
            elif kind == 6:
                inner = a * b * np.exp(5 * u - 3)
            elif kind == 7:
                inner = b * np.exp(8 * u - 5)
            elif kind == 8:
                inner = np.exp(a + b * (8 * u - 4))
            else:
                inner = a + b * (100 * u - 50)
            x = np.concatenate([edge, inner])
            xs.append(x)
            ys.append(np.stack([np.full(x.size, kind), np.full(x.size, a), np.full(x.size, b)]))
    return np.concatenate(xs), np.concatenate(ys, 1)


BM_WORDS = (0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF)


def box_muller_args():
    rng = np.random.default_rng(14)
    w = rng.integers(0, 2 ** 32, (2, 100000)).astype(np.float64)
    sp = np.array([(a, b) for a in BM_WORDS for b in BM_WORDS], np.float64).T
    x, where = pack(dict(random=w[0], specials=sp[0]))
    return x, np.concatenate([w[1], sp[1]])[None], where


def all_cases():
    """{name: (fn, x, y, where)} -- the whole run, one launch per entry"""
    c = {}
    for name, f in (("exp_nonpos", exp_nonpos_args), ("recip_pos", recip_pos_args), ("phi_table", phi_table_args),
                    ("log_phi_neg", log_phi_neg_args)):
        x, where = f()
        c[name] = (FN[name], x, None, where)
    x, where = softplus_args()
    c["softplus_fast"] = (FN["softplus_fast"], x, None, where)
    c["softplus_tab"] = (FN["softplus_tab"], x, None, where)
    for name in LBA_NA:
        x, y, where = lba_args(name)
        c[name] = (FN[name], x, y, where)
    x, y = prior_args()
    c["prior_term"] = (FN["prior_term"], x, y, {})
    x, y, where = box_muller_args()
    c["box_muller"] = (FN["box_muller"], x, y, where)
    return c


# ---- references -----------------------------------------------------------------------------------------------------------------
def _mp():
    import mpmath
    mpmath.mp.dps = 40
    return mpmath


def exp_ref(a):
    """exp(max(a, -700)) in 80-bit arithmetic (the helper's clamp is part of its definition)"""
    return np.exp(np.maximum(np.asarray(a, np.float64), -700.0).astype(ld))


def softplus_ref(x):
    x = np.asarray(x, np.float64).astype(ld)
    return np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))


def recip_ref(x):
    return ld(1) / np.asarray(x, np.float64).astype(ld)


def rel_err(got, ref):
    """|got - ref| / |ref| as float64, formed in 80-bit arithmetic"""
    return np.abs((np.asarray(got, np.float64).astype(ld) - ref) / ref).astype(np.float64)


def to_float(v):
    """an mpf as the nearest double, +-inf where it is beyond the double range"""
    try:
        return float(v)
    except OverflowError:
        return INF if v > 0 else -INF


def phi_ref(z):
    """(Phi(z), phi(z)) at 40 digits: two lists of mpf (the differences are formed at 40 digits too: mp_abs_err)"""
    mp = _mp()
    zz = [mp.mpf(float(v)) for v in z]
    return [mp.ncdf(v) for v in zz], [mp.npdf(v) for v in zz]


def log_phi_neg_ref(z):
    """log Phi(-z) at 40 digits: list of mpf"""
    mp = _mp()
    return [mp.log(mp.ncdf(-mp.mpf(float(v)))) for v in z]


def mp_abs_err(got, ref):
    """|got - ref| with the difference formed at 40 digits -> float64"""
    mp = _mp()
    return np.array([float(abs(mp.mpf(float(g)) - r)) for g, r in zip(got, ref)])


EPS_P, EPS_PHI = 2.5e-16, 3e-16  # the table's bars for Phi and for phi (tests/test_tables.py)


def lba_check(dev, rt, y, na):
    """One trial per row against make_golden.py's formulas at 40 digits.  Returns (err, base, kpart, ref): err = |dev - max(ref,
    1e-10)|, and the bound is base + K kpart (see test_gpu_device_math.test_lba_trial*), all from the reference alone:
        accumulator a with arguments n1 = (b - A - t v)/t, n2 = (b - t v)/t, factor p [c1 Phi(n1) + c2 Phi(n2) -+ (phi(n1) - phi(n2))]
            winner: p = 1/A, c = (-v, v)     loser: p = t/A, c = (-n1, n2)
        E_a = EPS_P p (|c1| + |c2|) + 2 EPS_PHI p  +  K 2^-53 M_a,   M_a = p sum_i (|c_i| Phi_i + phi_i + n_i^2 phi_i)
        product: |ref| (sum_a E_a / |factor_a| + na EPS_P / (1 - p_neg))
    (|ref| E_a / |factor_a| is formed as E_a times the other factors, so a factor of 0 divides nothing.)"""
    mp = _mp()
    n = len(rt)
    err, base, kpart, refs = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
    eP, eF, u, floor_ = mp.mpf(EPS_P), mp.mpf(EPS_PHI), mp.mpf(2) ** -53, mp.mpf(1e-10)
    for i in range(n):
        d = float(dev[i])
        tau = mp.mpf(float(y[7, i]))
        t = mp.mpf(float(rt[i])) - tau if rt[i] == rt[i] else mp.mpf(0)
        if not t > mp.mpf(1e-300):
            err[i] = abs(d) if d == d else INF  # the factor is exactly 0
            continue
        c, A, k = int(y[0, i]), mp.mpf(float(y[5, i])), mp.mpf(float(y[6, i]))
        b = A + k
        fac, e0, e1, pneg = [], [], [], mp.mpf(1)
        for a in range(na):
            v = mp.mpf(float(y[1 + a, i]))
            n1, n2 = (b - A - t * v) / t, (b - t * v) / t
            P1, P2, f1, f2 = mp.ncdf(n1), mp.ncdf(n2), mp.npdf(n1), mp.npdf(n2)
            if a + 1 == c:
                p, c1, c2 = 1 / A, v, v
                fac.append(p * (v * (P2 - P1) + (f1 - f2)))
            else:
                p, c1, c2 = t / A, n1, n2
                fac.append(p * ((n2 * P2 - n1 * P1) - (f1 - f2)))
            e0.append(eP * p * (abs(c1) + abs(c2)) + 2 * eF * p)
            e1.append(u * p * (abs(c1) * P1 + abs(c2) * P2 + f1 + f2 + n1 * n1 * f1 + n2 * n2 * f2))
            pneg *= mp.ncdf(-v)
        norm = 1 - pneg
        ref = mp.fprod(fac) / norm
        others = [mp.fprod([abs(fac[q]) for q in range(na) if q != a]) / norm for a in range(na)]
        base[i] = float(mp.fsum(e0[a] * others[a] for a in range(na)) + abs(ref) * na * eP / norm)
        kpart[i] = float(mp.fsum(e1[a] * others[a] for a in range(na)))
        refs[i] = float(ref)
        err[i] = float(abs(mp.mpf(d) - max(ref, floor_))) if np.isfinite(d) else INF
    return err, base, kpart, refs


def prior_ref(kind, a, b, x):
    """the log-density of prior `kind`(a, b) at x, 40 digits: (value, sum of the magnitudes of its terms); value is -inf outside the
    support, and None at Gamma's x = 0 (pinned apart); Beta at 0 and 1 as the device's form has it"""
    mp = _mp()
    lo, hi = prior_support(kind, a, b)
    if not (lo <= x <= hi) or (kind == 8 and x == 0.0):
        return -INF, 0.0
    if kind == 6 and x == 0.0:
        return None, 0.0
    if kind == 4 and x in (0.0, 1.0):  # the term whose exponent is 0 is dropped, as the device drops it; otherwise 0^(e) decides
        e = (a if x == 0.0 else b) - 1.0
        if e != 0.0:
            return (INF if e < 0 else -INF), 0.0
        o = mp.mpf(b if x == 0.0 else a)
        terms = [-mp.loggamma(1), -mp.loggamma(o), mp.loggamma(1 + o)]
        return mp.fsum(terms), to_float(mp.fsum(abs(t) for t in terms))
    a, b, x = mp.mpf(a), mp.mpf(b), mp.mpf(x)
    half_log2pi, logpi = mp.log(2 * mp.pi) / 2, mp.log(mp.pi)
    if kind == 1:
        terms = [-half_log2pi, -mp.log(b), -((x - a) / b) ** 2 / 2]
    elif kind == 2:
        terms = [-logpi, -mp.log(b), -mp.log1p(((x - a) / b) ** 2), -mp.log(1 - (mp.atan((0 - a) / b) / mp.pi + mp.mpf(0.5)))]
    elif kind == 3:
        terms = [-mp.log(b - a)]
    elif kind == 4:
        terms = [(a - 1) * mp.log(x), (b - 1) * mp.log1p(-x), -mp.loggamma(a), -mp.loggamma(b), mp.loggamma(a + b)]
    elif kind == 6:
        terms = [(a - 1) * mp.log(x), -x / b, -a * mp.log(b), -mp.loggamma(a)]
    elif kind == 7:
        terms = [-mp.log(b), -x / b]
    elif kind == 8:
        terms = [-mp.log(b), -half_log2pi, -mp.log(x), -((mp.log(x) - a) / b) ** 2 / 2]
    else:
        terms = [-logpi, -mp.log(b), -mp.log1p(((x - a) / b) ** 2)]
    return mp.fsum(terms), to_float(mp.fsum(abs(t) for t in terms))


def box_muller_ref(w0, w1):
    """(rad cos 2 pi u1, rad sin 2 pi u1, rad), rad = sqrt(-2 log(1 - u0)), u = (w + 1/2) / 2^32: lists of mpf"""
    mp = _mp()
    out = []
    for a, b in zip(w0, w1):
        u0, u1 = (mp.mpf(int(a)) + mp.mpf(0.5)) / 2 ** 32, (mp.mpf(int(b)) + mp.mpf(0.5)) / 2 ** 32
        rad = mp.sqrt(-2 * mp.log(1 - u0))
        out.append((rad * mp.cospi(2 * u1), rad * mp.sinpi(2 * u1), rad))
    return out


def box_muller_ref_ld(w0, w1):
    """the same in 80-bit arithmetic, for every point: (x, y, rad)"""
    u0, u1 = (np.asarray(w0).astype(ld) + ld(0.5)) / ld(2 ** 32), (np.asarray(w1).astype(ld) + ld(0.5)) / ld(2 ** 32)
    rad = np.sqrt(-2 * np.log1p(-u0))
    # sin / cos of 2 pi u1 through the reduced angle (u1 - round(2 u1)/2 is exact): the argument stays below pi/2
    q = np.rint(4 * u1)
    r = (u1 - q / 4) * (2 * ld("3.14159265358979323846264338327950288"))
    s, c = np.sin(r), np.cos(r)
    k = q.astype(np.int64) & 3
    cs = np.where(k == 0, c, np.where(k == 1, -s, np.where(k == 2, -c, s)))
    sn = np.where(k == 0, s, np.where(k == 1, c, np.where(k == 2, -s, -c)))
    return rad * cs, rad * sn, rad


# ---- the stand-in: every helper in its libm form (float64) ------------------------------------------------------------------------
def _lba_numpy(rt, y, na):
    from scipy.special import ndtr
    pdf = lambda v: np.exp(-0.5 * v * v) / np.sqrt(2 * np.pi)
    with np.errstate(all="ignore"):
        t = rt - y[7]
        A, b = y[5], y[5] + y[6]
        den, pneg = np.ones_like(rt), np.ones_like(rt)
        for a in range(na):
            v = y[1 + a]
            n1, n2 = (b - A - t * v) / t, (b - t * v) / t
            win = (1 / A) * (v * (ndtr(n2) - ndtr(n1)) + (pdf(n1) - pdf(n2)))
            lose = (t / A) * ((n2 * ndtr(n2) - n1 * ndtr(n1)) - (pdf(n1) - pdf(n2)))
            den = den * np.where(y[0] == a + 1, win, lose)
            pneg = pneg * ndtr(-v)
        den = den / (1 - pneg)
        return np.where((t > 1e-300) & (den == den), np.maximum(den, 1e-10), 0.0)


def standin(cases):
    """[(fn, x, y)] -> [(fn, out[2, n])] as the probe answers, from numpy / scipy in float64"""
    from scipy.special import log_ndtr, ndtr
    outs = []
    with np.errstate(all="ignore"):
        for fn, x, y in cases:
            o = np.zeros((2, x.size))
            if fn == FN["exp_nonpos"]:
                o[0] = np.exp(np.fmax(x, -700.0))
            elif fn in (FN["softplus_fast"], FN["softplus_tab"]):
                o[0] = np.fmax(x, 0.0) + np.log1p(np.exp(np.fmax(-np.abs(x), -700.0)))
            elif fn == FN["recip_pos"]:
                o[0] = 1.0 / x
            elif fn == FN["phi_table"]:
                z = np.fmin(np.fmax(x, -PHI_HALF), PHI_HALF) / PHI_S
                o[0], o[1] = np.exp(-0.5 * z * z) / np.sqrt(2 * np.pi) / PHI_S, ndtr(z)
            elif fn == FN["log_phi_neg"]:
                o[0] = log_ndtr(-np.fmax(x, -8.5))
            elif fn in (FN["lba2"], FN["lba3"], FN["lba_rt4"]):
                o[0] = _lba_numpy(x, y, {FN[k]: v for k, v in LBA_NA.items()}[fn])
            elif fn == FN["prior_term"]:
                o[0] = [to_float(v) if v is not None else NAN for v in (prior_ref(int(k), a, b, xx)[0] for xx, k, a, b in zip(x, *y))]
            elif fn == FN["box_muller"]:
                rad = np.sqrt(-2 * np.log1p(-(x + 0.5) / 2 ** 32))
                o[0], o[1] = rad * np.cos(2 * np.pi * (y[0] + 0.5) / 2 ** 32), rad * np.sin(2 * np.pi * (y[0] + 0.5) / 2 ** 32)
            else:
                raise KeyError(fn)
            outs.append((fn, o))
    return outs
