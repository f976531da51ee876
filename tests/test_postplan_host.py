"""csrc/demc_postplan.hpp -- the history window, the two small history rules and the planners of demc_summarize, demc_quantiles
and demc_covariance -- is host-only code: tests/postplan_host.cpp, a program of its own, holds it to the project's own statements
(DESIGN.md 5.5-5.7), to brute force written by other means and to every refusal's text.  Built with the address and
undefined-behaviour sanitizers, with -ffp-contract=off as the library is (the rank arithmetic of plan_quantiles depends on it), and
run once.  No GPU, no HIP runtime, and no ROCm include path: that the program compiles is the proof that the header is host-only.

The same program's --dump mode ties the Python restatements of this arithmetic -- geometry() of test_summary_host.py,
test_quantile_host.py and test_cov_host.py, targets() and hist_ld(), which the GPU tests import to assert the geometry a case was
chosen for -- to the code that launches: plans(), constants()."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "differentialevolutionmcmc.jl_amd", "csrc")


@functools.lru_cache(maxsize=None)
def program():
    """the program, built once per session"""
    tmp = tempfile.mkdtemp(prefix="postplan_host_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    exe = os.path.join(tmp, "postplan_host")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off",
                            "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(ROOT, "tests", "postplan_host.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    return exe


def _value(text):
    if "," in text or text == "":
        return [_value(t) for t in text.split(",")] if text else []
    return float.fromhex(text) if "x" in text else int(text)


def plans(requests):
    """one dict per request line (tests/postplan_host.cpp says what a line is): the fields of the plan, or refused and message"""
    run = subprocess.run([program(), "--dump"], input="\n".join(requests) + "\n", capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and not run.stderr, run.stdout[-2000:] + run.stderr
    lines = run.stdout.splitlines()
    assert len(lines) == len(requests), (len(lines), len(requests))
    out = []
    for req, line in zip(requests, lines):
        assert line[0] == req[0], (req, line)
        head, _, message = line.partition(" message=")
        d = {k: _value(v) for k, v in (tok.split("=", 1) for tok in head.split()[1:])}
        for k in ("slots", "lds_bytes", "rank", "gamma", "ia", "ib", "table"):  # (lists even when they hold one value)
            if req[0] in "QC" and k in d and not isinstance(d[k], list):
                d[k] = [d[k]]
        if message:
            d["message"] = message
        out.append(d)
    return out


def constants():
    """the k* constants of the header and the two public caps, as the compiler sees them"""
    return plans(["const"])[0]


def summary_request(n, P, D, max_lag=0, rho_len=0, wants_rho=False):
    return f"S {n} {P} {D} {max_lag} {rho_len} {int(wants_rho)}"


def quantile_request(N, D, ld, probs):
    return f"Q {N} {D} {ld} " + " ".join(float(p).hex() for p in probs)


def cov_request(N, D, cols=None):
    return f"C {N} {D} " + " ".join(str(c) for c in cols or ())


def test_plans_under_the_sanitizers():
    run = subprocess.run([program()], capture_output=True, text=True, timeout=300)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert "postplan ok" in run.stdout and "runtime error" not in run.stderr, run.stdout + run.stderr[-4000:]


def test_plans_are_written_in_the_host_only_header():
    """demc_postplan.hpp knows no HIP and no handle; the library reads no environment; the three argument records are one; the
    refusals of the window and of the plans are written in the header only; each planner is called exactly once."""
    import re
    header = open(os.path.join(CSRC, "demc_postplan.hpp")).read()
    for word in ("hip", "ALLOC", "demc_handle"):
        assert word not in header, word
    sources = {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".cpp", ".hpp")) or f == "Makefile"}
    for name, text in sources.items():
        assert "getenv" not in text, name
        for word in ("SumArgs", "QArgs", "CovArgs"):
            assert word not in text, (name, word)
    runtime = sources["demc_hip.cpp"]
    texts = re.findall(r'"((?:[^"\\]|\\.)*)"', re.sub(r"//.*|static_assert\(.*", "", header))
    refusals = [t for t in texts if " " in t and not t.endswith((".h", ".hpp"))]
    assert len(refusals) == 15, refusals  # the history, three windows, three sharded handles, too many rows (2), probs (2), columns (4)
    for t in refusals:
        assert t not in runtime, t
        assert sum(text.count('"' + t + '"') for text in sources.values()) == 1, t
    for call in ("plan_summary(", "plan_quantiles(", "plan_cov(", "history_cell_stride("):
        assert runtime.count(call) == 1, call
        assert sum(text.count(call) for name, text in sources.items() if name not in ("demc_hip.cpp", "demc_postplan.hpp")) == 0, call
    assert runtime.count("history_stage_rows(") == 2 and "64 << 20" not in runtime  # the two history copies
    for unit in ("demc_summary.cpp", "demc_quantile.cpp", "demc_cov.cpp"):  # the common tail is written once, in demc_devmem.hpp
        assert sources[unit].count("finish(who, st,") == 1 and "hipStreamSynchronize" not in sources[unit], unit


def test_python_restatements_are_the_plans():
    """geometry(), targets() and hist_ld() of the three host test modules against the planners, on a grid that holds every shape a
    check_geometry(...) of the GPU tests names"""
    import test_cov_host as C
    import test_gpu_cov as GC
    import test_gpu_quantile as GQ
    import test_gpu_summary as GS
    import test_quantile_host as Q
    import test_summary_host as S

    # ---- hist_ld
    Ds = list(range(1, 80)) + [600]
    got = plans([f"L {D} {k}" for D in Ds for k in (0, 1)])
    assert [g["ld"] for g in got] == [Q.hist_ld(D, bool(k)) for D in Ds for k in (0, 1)]

    # ---- demc_summarize: (n, P, D)
    shapes = {(n, G * Np, D) for n, G, Np, D, *_ in GS.LARGE.values()} | {(18305, 64, 6), (16, 8, 63), (16, 8, 70), (1000, 4096, 32), (200, 8, 2)}
    shapes |= {(n, 4, 1) for n in (8064, 8065, 18304, 18305)}
    shapes |= {(n, P, D) for n in (1, 2, 3, 4, 5, 64, 65, 128, 129, 130, 1000, 3968, 3969, 8064, 8065, 18304, 18305, 40000) for P in (3, 8, 1024, 1025) for D in (1, 2, 7, 33)}
    shapes = sorted(shapes)
    for (n, P, D), p in zip(shapes, plans([summary_request(*s) for s in shapes])):
        g = S.geometry(n, P, D)
        mode = "global" if not p["lds"] else "lds64" if p["lds_bytes"] <= S.SUM_LDS_SMALL else "lds144"
        assert (g["mode"], g["JT"], len(g["tiles"]), g["workers"], g["lag_blocks"]) == (mode, p["JT"], p["tiles"], p["workers"], p["lag_blocks"]), (n, P, D, g, p)
        assert sum(g["tiles"]) == D + 2 and max(g["tiles"]) == p["JT"] and g["chains_per_worker_max"] == -(-P // p["workers"])

    # ---- demc_quantiles: (n, P, D, ld, probs)
    shapes = {(n, P, D, D, Q.PROBS) for n, P, D, _ in GQ.GEOMETRY.values()} | {(16, 8, 62, 62, Q.PROBS), (20, 8, 9, 16, Q.PROBS), (1000, 4096, 32, 32, Q.DEFAULT),
                                                                                 (1000, 24, 2, 2, Q.DEFAULT), (4, 4, 70, 70, Q.PROBS), (1, 1, 3, 3, Q.PROBS)}
    shapes |= {(n, P, D, Q.hist_ld(D, pad), probs) for n in (1, 2, 3, 7, 129, 961) for P in (1, 8, 24) for D in (1, 2, 7, 9, 17, 33, 63, 70) for pad in (False, True)
               for probs in (Q.DEFAULT, Q.PROBS, (0.5,), (0.0, 1.0), (1e-9, 0.999, 0.1, 0.9))}
    shapes = sorted(shapes)
    for (n, P, D, ld, probs), p in zip(shapes, plans([quantile_request(n * P, D, ld, probs) for n, P, D, ld, probs in shapes])):
        g = Q.geometry(n, P, D, ld, probs)
        assert (g["cells_per_chunk"], g["chunks"], g["workgroups"], g["targets"], g["passes"]) == (p["cpi"], p["chunks"], p["W"], p["T"], len(p["slots"])), (n, P, D, ld, g, p)
        assert g["first_pass_slots"] == p["slots"][0] and set(p["slots"][1:]) == {g["later_slots"]}, (n, P, D, ld, g, p)
        assert p["lds_bytes"] == [s * 257 * 4 for s in p["slots"]] and g["first_pass_direct"] == max(0, p["n_series"] - p["slots"][0])
        assert Q.targets(n * P, probs) == p["rank"], (n, P, probs)

    # ---- demc_covariance: (n, P, D, ld, K); which K series are selected does not enter the geometry
    shapes = {(n, P, D, D, D + 2) for n, P, D, _ in GC.GEOMETRY.values()} | {(N // P, P, K, K, K) for N, P in ((24, 8), (2051, 7)) for K in (4, 17, 34, 64)}
    shapes |= {(n, P, 2, 2, 4) for n, P in ((1, 3), (1, 5), (1, 7), (8, 8), (13, 5))} | {(20, 8, 9, 16, 11), (3, 4, 600, 600, 64), (16, 8, 62, 62, 64), (1000, 4096, 32, 32, 34),
                                                                                         (1000, 24, 2, 2, 4), (1, 1, 62, 62, 64), (1, 1, 2, 2, 1)}
    shapes |= {(n, P, 62, 62, K) for n in (1, 2, 64, 65, 32769) for P in (1, 8) for K in (1, 15, 16, 17, 32, 33, 48, 49, 64)}
    shapes = sorted(shapes)
    for (n, P, D, ld, K), p in zip(shapes, plans([cov_request(n * P, D, range(D + 2 - K, D + 2)) for n, P, D, ld, K in shapes])):
        g = C.geometry(n, P, D, ld, K)
        assert (g["blocks"], g["tiles"], g["chunks"], g["workers"], g["partial"]) == (p["NB"], p["tiles"], p["chunks"], p["W"], p["partial"]), (n, P, D, K, g, p)
        assert g["scratch_bytes"] == 8 * (p["n_part1"] + p["n_mhat"] + p["n_part2"] + p["n_mean"] + 2 * p["n_mat"]) + 4 * p["n_cols"]
        assert p["table"] == list(range(D + 2 - K, D + 2)) + [-1] * (64 - K) and p["K"] == K
