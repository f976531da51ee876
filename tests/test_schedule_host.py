"""csrc/demc_schedule.hpp -- what a demc_step call does iteration by iteration: the host's re-draws of the device's coins, the
refusals of a step call, the segments, the sweeps and colour phases, the overlapped exchange's partition, the frozen-sweep launch
order -- and csrc/demc_philox.hpp under it are host-only code: tests/schedule_host.cpp, a program of its own, holds them to every
refusal's text and to their edges.  Built with the address and undefined-behaviour sanitizers, with -ffp-contract=off as the
library is, and run once.  No GPU, no HIP runtime, and no ROCm include path: that the program compiles is the proof that both
headers are host-only.

The same program's --dump mode is compared here with references written by other means: the oracle's alpha coin and select_groups
(independent C), a numpy restatement of the frozen order over weighted_pick_cases.philox_blocks (held to the oracle's Philox), and
a brute-force loop over the segment rules as DESIGN.md states them ("The schedule of a step call")."""
import atexit
import functools
import itertools
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "differentialevolutionmcmc.jl_amd", "csrc")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

NONE, LOCAL, EXCHANGE, OVERLAPPED = range(4)
SEEDS = (1, 7, 0x123456789ABCDEF0, 2 ** 63 + 5)  # (two with bits above bit 32: the key's second word)
SEG_SEED, SEG_ALPHA = 0x5DEECE66D00000B, 0.02  # iterations 1..200: at least three migrations and a gap longer than 64 (asserted below)
FROZEN_SEED = 0x9E3779B97F4A7C1C  # at beta = 0.1 some sweep has a mutating group that is not group 0 (asserted below)


SANITIZERS = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


@functools.lru_cache(maxsize=None)
def program(sanitized=True):
    """the program, built once per session: under the sanitizers for the CPU tests of this module; the same line without them for
    the GPU tests that only ask its --dump mode (no sanitizer runs beside a GPU)"""
    tmp = tempfile.mkdtemp(prefix="schedule_host_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    exe = os.path.join(tmp, "schedule_host")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g"] + (SANITIZERS if sanitized else []) + ["-ffp-contract=off",
                            "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(ROOT, "tests", "schedule_host.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    return exe


def dump(requests, sanitized=True):
    """one answer per request line (tests/schedule_host.cpp says what a line is): a list of ints, or of (run, migrate) for `seg`"""
    run = subprocess.run([program(sanitized), "--dump"], input="\n".join(requests) + "\n", capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and not run.stderr, run.stdout[-2000:] + run.stderr
    lines = run.stdout.splitlines()
    assert len(lines) == len(requests), (len(lines), len(requests))
    out = []
    for req, line in zip(requests, lines):
        what, _, body = line.partition(" ")
        assert what == req.split()[0], (req, line)
        items = [t for t in body.split(",") if t]
        out.append([tuple(int(x) for x in t.split(":")) for t in items] if what == "seg" else [int(t) for t in items])
    return out


def seg_request(seed, alpha, n_groups_total, n_groups, iter0, n_iters, with_migration=True, per_phase=False, cap=1024, own_comm=False,
                overlap=False, replay=False, replayed_step=False, u_step=0.0, history=False, set_size=0):
    return (f"seg {seed} {float(alpha)!r} {n_groups_total} {n_groups} {iter0} {n_iters} {int(with_migration)} {int(per_phase)} {cap} {int(own_comm)} "
            f"{int(overlap)} {int(replay)} {int(replayed_step)} {float(u_step)!r} {int(history)} {set_size}")


def segments(sanitized=True, **kw):
    """[(run, migrate)] of one call, as the runtime walks it (the GPU tests count launches against it, with sanitized=False)"""
    return dump([seg_request(**kw)], sanitized)[0]


def oracle_coin(seed, alpha, n_groups_total):
    from oracle import oracle as O
    cfg = O.make_config(n_groups=n_groups_total, n_groups_total=n_groups_total, alpha=alpha, seed=seed)
    L = O.lib()
    return lambda it: bool(L.orc_migration_due(O.C.byref(cfg), it))


def test_schedule_under_the_sanitizers():
    run = subprocess.run([program()], capture_output=True, text=True, timeout=300)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert "schedule ok" in run.stdout and "runtime error" not in run.stderr, run.stdout + run.stderr[-4000:]


def test_schedule_is_written_in_the_host_only_header():
    """the two headers know no HIP and no handle; each refusal of a step call is written in demc_schedule.hpp alone; the run rule is
    written once -- the runtime asks the coin only through its C wrapper and walks a call only through next_segment"""
    schedule = open(os.path.join(CSRC, "demc_schedule.hpp")).read()
    philox = open(os.path.join(CSRC, "demc_philox.hpp")).read()
    for word in ("hip", "demc_handle"):
        assert word not in schedule and word not in philox, word
    assert re.findall(r"#include [<\"]([^>\"]+)", philox) == ["stdint.h"]
    sources = {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".cpp", ".hpp"))}
    runtime = sources["demc_hip.cpp"]
    code = re.sub(r"//.*", "", schedule)
    texts = [re.sub(r'"\s*"', "", m) for m in re.findall(r'Refusal\{DEMC_EINVAL,\s*("(?:[^"\\]|\\.)*"(?:\s*"(?:[^"\\]|\\.)*")*)\}', code)]
    texts = [t[1:-1] for t in texts]
    assert len(texts) == 9, texts  # the model, the iteration, two of the history; a subset under history; its replay, its indices; the set, the communicator
    for t in texts:
        first_piece = t[:40]
        assert first_piece not in runtime, t
        assert sum(text.count(first_piece) for text in sources.values()) == 1, t
    # the run rule: no loop over the coin outside the header, and the header's own is run_length alone
    due_lines = [ln.strip() for ln in runtime.splitlines() if "migration_due" in re.sub(r"//.*", "", ln)]
    assert due_lines == ["int32_t demc_migration_due(const demc_config* cfg, int64_t iter) { return cfg && migration_due(*cfg, iter) ? 1 : 0; }"], due_lines
    assert runtime.count("next_segment(") == 2  # step_body and demc_multi_step
    assert len(re.findall(r"\bwhile\b.*due\(", code)) == 1 and code.count("run_length(") == 3  # its definition and next_segment's two uses
    assert sum(text.count("draw_block(") for name, text in sources.items() if name == "demc_hip.cpp") == 0  # no host draw outside the header
    for gone in ("glist_buf", "glist_pin", "glist_ev", "glist_next", "frozen_order_d", "frozen_order_cap", "frozen_order_pin", "frozen_order_ev",
                 "h->frozen_iter0", "h->frozen_iters"):  # the eleven fields the two staging mechanisms took: one owner now (StagedList)
        assert gone not in runtime, gone


def test_coins_against_the_oracle():
    """the alpha coin and select_groups: every iteration 1..200, seeds with and without high bits, 1 to 64 groups"""
    from oracle import oracle as O
    cases = [(seed, ng) for seed in SEEDS for ng in (1, 2, 3, 5, 64)]
    alpha = 0.3
    coins = dump([f"coin {seed} {alpha!r} {ng} 1 201" for seed, ng in cases])
    groups = dump([f"groups {seed} {ng} {it}" for seed, ng in cases for it in range(1, 201)])
    fired = 0
    for i, (seed, ng) in enumerate(cases):
        orc = O.Oracle(n_groups=ng, Np=4, D=1, alpha=alpha, seed=seed)
        want = [int(orc.migration_due(it)) for it in range(1, 201)]
        assert coins[i] == want, (seed, ng)
        fired += sum(want)
        for it in range(1, 201):
            sel = groups[i * 200 + it - 1]
            assert sel == [int(g) for g in orc.migration_plan(it)], (seed, ng, it)
            if ng == 1:
                assert want[it - 1] == 0 and sel == []
            if ng == 2:
                assert sorted(sel) == [0, 1]
        orc.close()
    assert fired > 100  # (the coins do fire)


def frozen_reference(seed, beta, n_groups, group_offset, frozen, iter0, n_iters):
    """numpy: the coin of group g in sweep b of iteration t is block 0 of S_GROUP at entity group_offset + g; u53 <= beta first, stably"""
    import weighted_pick_cases as W
    out, mutating = [], []
    for t in range(iter0, iter0 + n_iters):
        for b, fr in enumerate(frozen):
            r = W.philox_blocks(seed, 2, b, t, group_offset + np.arange(n_groups), 0)
            mut = (W.u53_array(r[..., 0], r[..., 1]) <= beta) & fr
            g = np.arange(n_groups)
            out += list(g[mut]) + list(g[~mut])
            mutating.append(g[mut])
    return [int(x) for x in out], mutating


def test_frozen_order_against_numpy_philox():
    frozen = (True, False, True)  # 3 blocks, the middle one not frozen
    bits = sum(1 << b for b, fr in enumerate(frozen) if fr)
    cases = [(beta, G, off) for beta in (0.1, 1.0) for G in (1, 2, 7) for off in (0, 5)]
    got = dump([f"frozen {FROZEN_SEED} {beta!r} {G} {off} 3 {bits} 11 3" for beta, G, off in cases])
    for (beta, G, off), order in zip(cases, got):
        want, mutating = frozen_reference(FROZEN_SEED, beta, G, off, frozen, 11, 3)
        assert order == want, (beta, G, off)
        rows = np.asarray(order).reshape(3, 3, G)
        assert (rows[:, 1, :] == np.arange(G)).all()  # the block that is not frozen: the identity
        if beta == 1.0:
            assert (rows == np.arange(G)).all()  # everybody mutates: nobody overtakes
        elif G > 1:
            # the seed is chosen so that the order differs from the identity: somewhere a group other than group 0 mutates alone in front
            assert any(len(m) and m[0] != 0 for m in mutating), (G, off)
            assert (rows != np.arange(G)).any(), (G, off)


def brute_force(coin, iter0, n_iters, with_migration, per_phase, cap, sharded, overlap, replay, history, set_size):
    """DESIGN.md "The schedule of a step call", from the list of due iterations"""
    if set_size:
        with_migration, per_phase, cap, sharded, overlap = set_size > 1, False, None, True, False
    end = iter0 + n_iters
    due = [it for it in range(iter0, end) if with_migration and coin(it)]
    out, it = [], iter0
    while it < end:
        kind = NONE
        if it in due:
            kind = LOCAL if not sharded else OVERLAPPED if overlap and not replay and not history else EXCHANGE
        limits = [end - it] + [d - it for d in due if d > it][:1]
        if kind != OVERLAPPED:
            limits.append(1 if per_phase else cap if cap is not None else end - it)
        out.append((min(limits), kind))
        it += min(limits)
    return out


def test_segments_against_brute_force():
    coin = oracle_coin(SEG_SEED, SEG_ALPHA, 4)
    due = [it for it in range(1, 201) if coin(it)]
    gaps = np.diff([0] + due + [201])
    assert len(due) >= 3 and gaps.max() > 65, (due, gaps)  # three migrations, and a run longer than the streaming forms' cap of 64
    first, last = due[0], due[-1]
    free = ([0] + due)[int(gaps.argmax())] + 1  # the first iteration of the longest stretch without a coin
    calls = [(1, 200), (1, 0), (first, last - first + 1), (free, 64), (free, 65), (due[1], 1)]  # whole; empty; coin first and last; a run of the cap and one more
    requests, wants = [], []
    for (iter0, n), cap, with_migration, (ngt, ng, own_comm, overlap), (replay, u_step), history, set_size in itertools.product(
            calls, (1, 64, 1024), (True, False), ((4, 4, False, False), (4, 4, True, False), (8, 4, False, False), (8, 4, False, True), (4, 4, True, True), (4, 4, False, True)),
            ((False, 0.0), (True, SEG_ALPHA / 2), (True, SEG_ALPHA * 2)), (False, True), (0, 1, 2)):
        c = oracle_coin(SEG_SEED, SEG_ALPHA, ngt)
        this_coin = (lambda it, u=u_step: u <= SEG_ALPHA) if replay else c
        for per_phase in ((True, False) if cap == 1 else (False,)):  # (FORM_PHASE and the lean DE-MC_Z form both launch one iteration)
            requests.append(seg_request(SEG_SEED, SEG_ALPHA, ngt, ng, iter0, n, with_migration, per_phase, cap, own_comm, overlap, replay, replay, u_step, history, set_size))
            wants.append(brute_force(this_coin, iter0, n, with_migration, per_phase, cap, ngt != ng or own_comm, overlap, replay, history, set_size))
    got = dump(requests)
    kinds = set()
    for req, g, w in zip(requests, got, wants):
        assert g == w, (req, g, w)
        n = int(req.split()[6])
        assert sum(run for run, _ in g) == n and all(run >= 1 for run, _ in g), req  # the segments tile [iter0, end)
        kinds |= {k for _, k in g}
    assert kinds == {NONE, LOCAL, EXCHANGE, OVERLAPPED}
    # the edges by name: a run exactly as long as the cap is one launch, one iteration longer is two
    assert segments(seed=SEG_SEED, alpha=SEG_ALPHA, n_groups_total=4, n_groups=4, iter0=free, n_iters=64, cap=64) == [(64, NONE)]
    assert segments(seed=SEG_SEED, alpha=SEG_ALPHA, n_groups_total=4, n_groups=4, iter0=free, n_iters=65, cap=64) == [(64, NONE), (1, NONE)]
    assert segments(seed=SEG_SEED, alpha=SEG_ALPHA, n_groups_total=4, n_groups=4, iter0=first, n_iters=last - first + 1, cap=1024)[0][1] == LOCAL
    assert segments(seed=SEG_SEED, alpha=SEG_ALPHA, n_groups_total=4, n_groups=4, iter0=first, n_iters=last - first + 1, cap=1024)[-1] == (1, LOCAL)
    # one group in total: no coin, replayed or not (alpha is 0)
    assert segments(seed=SEG_SEED, alpha=1.0, n_groups_total=1, n_groups=1, iter0=1, n_iters=50, cap=64) == [(50, NONE)]
