"""The two weighted picks of the sampler -- select_base (crossover.jl:282-289: the base particle of a crossover proposal inside
burn-in) and select_particle (migration.jl:64-70: the row a group sends away) -- as their DEFINITION, written once more by other
means: 50-digit arithmetic (mpmath), exact cumulative sums in index order, "first i with C_i >= u T".  The oracle restates the rule
once (oracle/demc_oracle.c: cdf_fixed_order, select_base_stable, select_particle_stable) and the kernels six more times, each with
code of its own per pool size and a search of its own (binary search, two-level counts over 4 or 16 lanes, ballot counts, a count
reduced over four waves); tests/test_weighted_pick_host.py holds the oracle to this file on the CPU and
tests/test_gpu_weighted_pick.py the kernels.  Nothing here needs a GPU.

The rule.  Both picks are stabilised softmax draws, a documented deviation from the reference:
  base      e_j = exp(w_j - max w)     degenerate (the total is not a positive finite number: a NaN or +Inf weight, or all -Inf)
                                       -> min(int(u n), n - 1)
  particle  e_j = exp(min w - w_j)     degenerate (any weight -Inf or NaN, or all +Inf: the reference's normalised weights hold a
                                       NaN) -> the first argmin over the comparable entries, else 0 (its findmin fallback).
                                       Comparable: below +Inf (a NaN compares with nothing, and a walk that starts at +Inf with a
                                       strict < never stops at +Inf), so a NaN among weights that are otherwise all +Inf gives 0.
and the pick is the first i with C_i >= u T, C the cumulative sums of e and T = C_{n-1}; the walk stops at n - 1 whatever u T is.

The ambiguity band.  The engines form C in floating point, in the fixed three-level order (sequential inside quads of four
entries, over the four quad totals of a chunk of 16, over the chunk totals).  A cumulative weight cdf[i] is then reached through
at most 3 additions inside its quad, 2 over the quad totals before it (the first is 0 + T_0, exact), 1 that joins the two, and
ceil(n/16) - 2 over the chunk totals before its chunk (again the first is exact) plus 1 that joins them: d = ceil(n/16) + 5
roundings, each at most 2^-53 of a partial sum, which is at most T.  Every e_j carries the error of exp, one ulp = 2^-52 of
itself, so together at most 2^-52 C_i.  Both sides of the comparison carry this -- cdf[i], and total = cdf[n-1] inside
t = fl(u total), u < 1 -- and the product rounds once more:
    |(cdf[i] - t) - (C_i - u T)| <= 2 (d 2^-53 + 2^-52) T + 2^-53 T = (ceil(n/16) + 7.5) 2^-52 T <= (ceil(n/16) + 8) 2^-52 T.
A pick whose u T lies farther than that from every boundary C_0 .. C_{n-2} (C_{n-1} is none: the walk stops there) is decided the
same way by every arithmetic within these bounds: UNIQUE.  Inside the band a pick is AMBIGUOUS and may fall on either side; `lo`
and `hi` of a Pick are the picks at the two ends of the band.  The tests allow no ambiguous case for any committed seed: a seed
that lands in the band is changed, never the band.  Two kinds of case are unique although a boundary is near, because the
floating-point cumulative weights and t are then exact: pattern (b) (one live entry: cdf is 0 before it and 1 from it on, t = u)
and pattern (d) on a power-of-two pool (equal weights: cdf is the integers, t = u n); there `<` against `<=` decides, which is
what the knife-edge uniforms are for.  The knife-edge uniforms 0, 2^-53 and 1 - 2^-53 are not seeds: on the other patterns they
may lie in the band (a leading weight of zero, a tail of denormal weights), and then anything from `lo` to `hi` is right.

What cannot be arranged: a uniform of a FREE-RUNNING lean kernel that lands exactly on a cumulative weight is a 2^-53 event per
draw; the comparison operator of the five lean restatements is therefore held only through patterns (b) and (d) with whatever
uniforms Philox hands out (u T never equals a C_i there), not on the knife edge.  The replay path puts the knife-edge uniforms
through the general kernel (k_propose) alone."""
import bisect
import collections
import math

import numpy as np
from mpmath import mp, mpf

DIGITS = 50
INF, NAN = float("inf"), float("nan")
SHIFT = -1.0e6          # every base pattern is shifted by this: any proposal then beats the current weight, in both schedules
GRID = 2.0 ** -20       # ... and every entry is a multiple of this, so the shift is exact (1e6 < 2^20: 40 bits of 53)
DROP = 800.0            # exp(-800) underflows to exactly 0.0 (the smallest denormal is exp(-744.44))
RAMP = 760.0            # a ramp down to -760 passes the denormal weights (exp(-708.4) .. exp(-744.4)) and ends in exact zeros

Pick = collections.namedtuple("Pick", "index dist lo hi degenerate")


def band(n):
    """half-width of the ambiguity band, as a fraction of the total (derivation: the module docstring)"""
    return (-(-n // 16) + 8) * 2.0 ** -52


def _cumulative(e):
    C, s = [], mpf(0)
    for x in e:
        s = s + x
        C.append(s)
    return C


def _first_at_least(C, t):
    """first i with C[i] >= t, else the last index (C is non-decreasing)"""
    return min(bisect.bisect_left(C, t), len(C) - 1)


class _Table:
    """the exact cumulative weights of one pool, formed once, asked for many uniforms"""

    def __init__(self, n, e=None, fallback=None):
        self.n, self.fallback = n, fallback
        if e is not None:
            self.C = _cumulative(e)
            self.T = self.C[-1]
            self.h = mpf(band(n)) * self.T

    def pick(self, u):
        n = self.n
        if self.fallback is not None:
            i = self.fallback(u)
            return Pick(i, INF, i, i, True)
        with mp.workdps(DIGITS):
            C, T = self.C, self.T
            t = mpf(u) * T
            i = _first_at_least(C, t)
            near = [abs(t - C[k]) for k in (i - 1, i) if 0 <= k <= n - 2]  # (C is sorted: the nearest boundary is one of these two)
            dist = float(min(near) / T) if near else INF
            return Pick(i, dist, _first_at_least(C, t - self.h), _first_at_least(C, t + self.h), False)


def exact_table_base(w):
    """select_base over the pool weights w: .pick(u) -> Pick(index, distance of u T to the nearest boundary as a fraction of T, the
    picks at the two ends of the ambiguity band, whether the degenerate branch answered)"""
    with mp.workdps(DIGITS):
        w = [float(x) for x in w]
        n = len(w)
        comparable = [x for x in w if not math.isnan(x)]
        m = mpf(max(comparable)) if comparable else mpf("-inf")
        e = [mp.exp(mpf(x) - m) for x in w]  # (inf - inf and anything with a NaN: NaN, as in floating point)
        T = _cumulative(e)[-1]
        if not (T > 0 and T < mpf("inf")):  # (a NaN total compares false twice)
            return _Table(n, fallback=lambda u: min(int(u * n), n - 1))
        return _Table(n, e)


def exact_table_particle(w):
    """select_particle over a group's weights w: .pick(u) -> Pick, as exact_table_base"""
    with mp.workdps(DIGITS):
        w = [float(x) for x in w]
        comparable = [(x, i) for i, x in enumerate(w) if x < INF]  # (a NaN compares with nothing, and nothing lies above +Inf)
        bad = any(not (x > -INF) for x in w)  # -Inf or NaN
        if bad or not comparable:
            i = min(comparable)[1] if comparable else 0  # (tuples: the first index among equal minima)
            return _Table(len(w), fallback=lambda u: i)
        m = mpf(min(comparable)[0])
        return _Table(len(w), [mp.exp(m - mpf(x)) for x in w])


def exact_pick_base(w, u):
    return exact_table_base(w).pick(u)


def exact_pick_particle(w, u):
    return exact_table_particle(w).pick(u)


def is_ambiguous(pick, n):
    return (not pick.degenerate) and pick.dist <= band(n)


# ---- the addressed draws -------------------------------------------------------------------------------------
S_STEP, S_PART, S_MIG = 1, 3, 6


def _block(seed, stream, sweep, it, entity, block):
    from oracle import oracle as O
    return O.philox([block, entity & 0xFFFFFFFF, it & 0xFFFFFFFF, (stream << 24) | (sweep & 0xFFFF)], [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF])


def u53(lo, hi):
    return float(((hi << 32) | lo) >> 11) * 2.0 ** -53


def mulhi(x, m):
    return (x * m) >> 32


def u_base(seed, it, sweep, global_slot):
    """select_base's uniform of a particle: PART block 0, words z and w"""
    r = _block(seed, S_PART, sweep, it, global_slot, 0)
    return u53(r[2], r[3])


def u_mig(seed, it, global_group):
    """select_particle's uniform of a group: MIG block 0, words x and y"""
    r = _block(seed, S_MIG, 0, it, global_group, 0)
    return u53(r[0], r[1])


def select_groups_ref(seed, it, ng):
    """select_groups (migration.jl:31-35): ns = 2 + mulhi(w2, ng - 1) of the ng groups, in order, by a partial Fisher-Yates whose
    word i is word i % 4 of block 1 + i // 4 of the STEP stream"""
    if ng < 2:
        return np.zeros(0, np.int32)
    ns = 2 + mulhi(_block(seed, S_STEP, 0, it, 0, 0)[2], ng - 1)
    perm = list(range(ng))
    r = None
    for i in range(ns):
        if i % 4 == 0:
            r = _block(seed, S_STEP, 0, it, 0, 1 + i // 4)
        j = i + mulhi(r[i % 4], ng - i)
        perm[i], perm[j] = perm[j], perm[i]
    return np.array(perm[:ns], np.int32)


def iteration_selecting(seed, ng, at_least, first=1):
    """the first iteration from `first` on whose select_groups takes at least `at_least` of the ng groups"""
    it = first
    while 2 + mulhi(_block(seed, S_STEP, 0, it, 0, 0)[2], ng - 1) < at_least:
        it += 1
    return it


# ---- weight patterns on a pool of n ------------------------------------------------------------------------------------------------
def _grid(x):
    return np.round(np.asarray(x, np.float64) / GRID) * GRID


def _typical(n, rng):
    return _grid(rng.normal(0.0, 3.0, n))


def live_positions(n):
    """pattern (b): where the one live entry sits -- the first entry, both sides of a quad, chunk and wave border, the last entry"""
    return sorted({j for j in (0, 3, 4, 15, 16, 63, 64, n - 1) if 0 <= j < n})


def base_patterns(n, seed):
    """[(name, w[n], unique)]: the weight patterns of a select_base pool.  `unique`: the floating-point cumulative weights AND t are
    exact (pattern b: total = 1; pattern d on a power-of-two pool: t = u n), so the answer is unique on the knife edge too; equal
    weights on another pool are exact up to the one rounding of u n, which the band covers.  Finite entries are multiples of 2^-20
    shifted by -1e6."""
    rng = np.random.default_rng([seed, n])
    out = [("a-normal", _typical(n, rng), False)]
    for j in live_positions(n):
        w = np.full(n, -DROP)
        w[j] = 0.0
        out.append((f"b-live{j}", w, True))
    ramp = -_grid(RAMP * np.arange(n) / (n - 1))
    out.append(("c-ramp", ramp, False))
    out.append(("c-ramp-up", ramp[::-1].copy(), False))  # (the same weights with the zeros and denormals in front)
    out.append(("d-equal", np.full(n, _grid(rng.normal(0.0, 3.0))), n & (n - 1) == 0))
    for name, sl in (("e-first", slice(0, 1)), ("e-last", slice(n - 1, n)), ("e-chunk", slice(0, 16))):
        if name == "e-chunk" and n <= 16:
            continue  # (a whole leading chunk only where entries remain behind it)
        w = _typical(n, rng)
        w[sl] = -INF
        out.append((name, w, False))
    out.append(("f-all-ninf", np.full(n, -INF), False))
    for name, v in (("g-nan", NAN), ("h-pinf", INF)):
        w = _typical(n, rng)
        w[int(rng.integers(0, n))] = v
        out.append((name, w, False))
    return [(name, w + SHIFT, unique) for name, w, unique in out]


def particle_patterns(n, seed):
    """the mirror images for select_particle (the small weights are the likely ones), and -- where the group is long enough -- two
    equal finite minima in different waves (70 and 300) with a NaN elsewhere: the first-index rule of the argmin"""
    out = [(name, -(w - SHIFT), unique) for name, w, unique in base_patterns(n, seed)]
    if n > 300:
        rng = np.random.default_rng([seed, n, 1])
        w = _typical(n, rng)
        w[[70, 300]] = w.min() - 1.0
        w[int(rng.choice([k for k in range(n) if k not in (70, 300)]))] = NAN
        out.append(("argmin-tie", w, False))
    return out


def knife_edge_uniforms(name, n):
    """uniforms on which the comparison operator decides: the two ends of [0, 1), and for equal weights on a power-of-two pool every
    k / n (cdf is the integers and t = k exactly: cdf[k-1] == t)"""
    us = [0.0, 2.0 ** -53, 1.0 - 2.0 ** -53]
    if name == "d-equal" and n & (n - 1) == 0:
        us += [k / n for k in range(n)]
    return us


def seeded_uniforms(n, seed, count=200):
    return np.random.default_rng([seed, n, 2]).random(count)


SIZES = (2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 600)
SEED = 20261020


def agrees(got, pick, unique, n):
    """whether an engine's index `got` is what the exact reference allows: the pick itself, or -- inside the ambiguity band of a case
    whose floating-point cumulative weights are not exact -- anything between the picks at the band's two ends"""
    if unique or not is_ambiguous(pick, n):
        return got == pick.index
    return pick.lo <= got <= pick.hi


# ---- the crossover proposal a pick leads to, formed here from the addressed draws (crossover.jl:154-172) ----------------------------
S_NOISE = 4


def philox_blocks(seed, stream, sweep, it, entity, block):
    """Philox4x32-10 over numpy arrays of entities and blocks -> uint32 [..., 4] (checked against oracle.philox on the CPU)"""
    entity, block = np.broadcast_arrays(np.asarray(entity, np.uint64), np.asarray(block, np.uint64))
    M32 = np.uint64(0xFFFFFFFF)
    c = [block & M32, entity & M32, np.full(entity.shape, it & 0xFFFFFFFF, np.uint64), np.full(entity.shape, (stream << 24) | (sweep & 0xFFFF), np.uint64)]
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & M32]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack(c, -1).astype(np.uint32)


def u53_array(lo, hi):
    return (((hi.astype(np.uint64) << np.uint64(32)) | lo.astype(np.uint64)) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def u_base_array(seed, it, sweep, global_slots):
    r = philox_blocks(seed, S_PART, sweep, it, global_slots, 0)
    return u53_array(r[..., 2], r[..., 3])


def crossover_proposals(seed, it, sweep, global_slots, pt, Pm, Pn, Pb, eps, cols=None, mask=None):
    """((Pt + g1 (Pm - Pn)) + g2 (Pb - Pt)) + b of random_gamma inside burn-in (crossover.jl:160-168), one row per slot, in the
    operand order both engines keep (a fixed sequence of correctly rounded + - *, so numpy's float64 gives the same bits):
    g1, g2 = 0.5 + 0.5 u from PART block 2, b_j = -eps + 2 eps u with u = (word + 1/2) 2^-32 from word j % 4 of NOISE block j / 4.
    `cols`: the scalars to form (all of them); `mask`: a block mask (reset!: scalars outside keep Pt's value)"""
    slots = np.asarray(global_slots, np.uint64)
    D = pt.shape[1]
    cols = np.arange(D) if cols is None else np.asarray(cols)
    rg = philox_blocks(seed, S_PART, sweep, it, slots, 2)
    g1 = (0.5 + (1.0 - 0.5) * u53_array(rg[:, 0], rg[:, 1]))[:, None]
    g2 = (0.5 + (1.0 - 0.5) * u53_array(rg[:, 2], rg[:, 3]))[:, None]
    words = philox_blocks(seed, S_NOISE, sweep, it, slots[:, None], (cols // 4)[None, :])  # [slots, cols, 4]
    wj = np.take_along_axis(words, np.broadcast_to((cols % 4)[None, :, None], words.shape[:2] + (1,)), 2)[..., 0]
    u = (wj.astype(np.float64) + 0.5) * (1.0 / 4294967296.0)
    b = -eps + (eps - (-eps)) * u
    pt, Pm, Pn, Pb = (x[:, cols] for x in (pt, Pm, Pn, Pb))
    prop = pt + (Pm - Pn) * g1
    prop = prop + (Pb - pt) * g2
    prop = prop + b
    if mask is not None:
        prop = np.where(np.asarray(mask)[cols][None, :] != 0, prop, pt)
    return prop


# ---- the crafted steps of tests/test_gpu_weighted_pick.py (formed here so that the CPU suite can hold their seeds to the band) ----
GPU_SEED = 20261021   # the Philox seed of every engine there: with it no uniform of any case lies inside the ambiguity band
POOLS = (4, 5, 15, 16, 17, 64, 65, 128, 129, 256, 257, 300)
# (groups, Np, schedule, history partners) of every select_base case: two_colour groups are odd, Np = 2 pool - 1, so that the
# crafted pool (the resting colour of phase 0, Np - Np / 2 entries) and the other colour differ; synchronous pools are whole groups
# (Np = 514: the one even group, where both colours must have 257 entries)
GPU_BASE_SHAPES = sorted({(2, 2 * p - 1, 2, False) for p in POOLS + (63, 127)} | {(2, p, 1, True) for p in POOLS + (255,)} |
                         {(1, 2 * p - 1, 2, False) for p in (64, 65, 256, 257)} | {(1, 514, 2, False)})


def pool_of(Np, schedule):
    """(pool_lo, pool size, the slots that move against it) of the crafted phase"""
    half = Np // 2
    return (half, Np - half, np.arange(half)) if schedule == 2 else (0, Np, np.arange(Np))


def crafted_step(seed, G, Np, schedule, n_init, k):
    """pattern k on the pools of G groups at iteration 1 + n_init + k -> (name, iteration, w[P], the global slots that move
    against the crafted pool, the slot of the exact base of each, unique).  Raises if a uniform lies inside the ambiguity band."""
    pool_lo, n, movers = pool_of(Np, schedule)
    name, _, unique = base_patterns(n, SEED)[k]
    it = 1 + n_init + k
    P = G * Np
    w = _typical(P, np.random.default_rng([k, 2])) + SHIFT
    gslot = (np.arange(G)[:, None] * Np + movers[None, :]).ravel()
    u = u_base_array(seed, it, 0, gslot)
    b = np.empty(gslot.size, np.int64)
    for g in range(G):
        wp = base_patterns(n, SEED + g)[k][1]
        w[g * Np + pool_lo: g * Np + pool_lo + n] = wp
        tb = exact_table_base(wp)
        for q in range(movers.size):
            pick = tb.pick(u[g * movers.size + q])
            if not unique and is_ambiguous(pick, n):
                raise AssertionError(f"{name}, Np = {Np}, schedule {schedule}: slot {gslot[g * movers.size + q]} is inside the band ({pick}); change GPU_SEED")
            b[g * movers.size + q] = g * Np + pool_lo + pick.index
    return name, it, w, gslot, b, unique
