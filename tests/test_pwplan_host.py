"""csrc/demc_pwplan.hpp -- the families, refusals, cell cap and planner of demc_pointwise_loglik and demc_waic -- is
host-only code: tests/pwplan_host.cpp, a program of its own, holds it to brute force written by other means and to every refusal's
text.  Built with the address and undefined-behaviour sanitizers, with -ffp-contract=off as the library is, and run once.  No GPU,
no HIP runtime, and no ROCm include path: that the program compiles is the proof that the header is host-only.

The same program's --dump mode ties geometry() below -- the Python restatement the GPU tests import to name the shapes a case was
chosen for -- to the code that launches."""
import atexit
import functools
import os
import re
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "differentialevolutionmcmc.jl_amd", "csrc")

PW_WG, PW_MIN_CHUNK, PW_TARGET_WG, PW_MAX_CHUNKS, PW_PARTIAL = 256, 64, 2048, 1024, 5
PW_MAX_CELLS = 1 << 27
FAMILY = dict(gaussian=0, mvn_iso=1, mvn_full=2, binomial=3, hier_binomial=4, hier_gaussian=5, lba=6, lnr=7, rastrigin=8, ode_lv=9, user=100, sim=101)


def geometry(N, S):
    """what demc_waic (and demc_pointwise_loglik, with S = its n rows) launches for N observations and S draws -> dict(tiles,
    chunks, chunk_len, last_chunk, workgroups)"""
    tiles = -(-N // PW_WG)
    want = max(1, min(max(1, PW_TARGET_WG // tiles), PW_MAX_CHUNKS, -(-S // PW_MIN_CHUNK)))
    chunk_len = -(-S // want)
    chunks = -(-S // chunk_len)
    return dict(tiles=tiles, chunks=chunks, chunk_len=chunk_len, last_chunk=S - (chunks - 1) * chunk_len, workgroups=tiles * chunks)


def constants_per_draw(family, n_acc=0, dp=0):
    return dict(gaussian=4, binomial=3, lnr=n_acc + 2, lba=2 * n_acc + 7, mvn_iso=dp + 3, mvn_full=dp + 1)[family]


@functools.lru_cache(maxsize=None)
def program():
    """the program, built once per session"""
    tmp = tempfile.mkdtemp(prefix="pwplan_host_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    exe = os.path.join(tmp, "pwplan_host")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off",
                            "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(ROOT, "tests", "pwplan_host.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    return exe


def plans(requests):
    """one dict per request line (tests/pwplan_host.cpp says what a line is): the fields of the plan, or refused and message"""
    run = subprocess.run([program(), "--dump"], input="\n".join(requests) + "\n", capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and not run.stderr, run.stdout[-2000:] + run.stderr
    lines = run.stdout.splitlines()
    assert len(lines) == len(requests), (len(lines), len(requests))
    out = []
    for line in lines:
        head, _, message = line.partition(" message=")
        d = {k: int(v) for k, v in (tok.split("=", 1) for tok in head.split()[1:])}
        if message:
            d["message"] = message
        out.append(d)
    return out


def request(call, family, N, S, D, direct=False, n_acc=0, d=0, dp=0):
    return f"P {call} {FAMILY[family]} {int(direct)} {N} {n_acc} {d} {dp} {S} {D}"


def test_plans_under_the_sanitizers():
    run = subprocess.run([program()], capture_output=True, text=True, timeout=300)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert "pwplan ok" in run.stdout and "runtime error" not in run.stderr, run.stdout + run.stderr[-4000:]


def test_plan_is_written_in_the_host_only_header():
    """demc_pwplan.hpp knows no HIP and no handle and adds nothing to demc_postplan.hpp; the refusals of the two calls are written in
    it only; the runtime gains two entry points that plan once each; the new unit ends through finish() like the others."""
    header = open(os.path.join(CSRC, "demc_pwplan.hpp")).read()
    for word in ("hip/", "hipStream", "ALLOC", "demc_handle", "getenv"):
        assert word not in header, word
    sources = {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".cpp", ".hpp"))}
    runtime = sources["demc_hip.cpp"]
    texts = re.findall(r'"((?:[^"\\]|\\.)*)"', re.sub(r"//.*", "", header))
    refusals = [t for t in texts if len(t) >= 28 and " " in t]  # (whole sentences, not the joints between two parts of one)
    assert len(refusals) >= 9, refusals
    for t in refusals:
        for name, text in sources.items():
            if name != "demc_pwplan.hpp":
                assert '"' + t + '"' not in text, (name, t)
    assert "pwplan" not in sources["demc_postplan.hpp"] and "waic" not in sources["demc_postplan.hpp"]
    assert runtime.count("plan_pointwise(") == 2  # one per entry point
    assert sum(text.count("plan_pointwise(") for name, text in sources.items() if name not in ("demc_hip.cpp", "demc_pwplan.hpp")) == 0
    unit = sources["demc_pointwise.cpp"]
    assert unit.count("finish(who, st,") == 2 and "hipStreamSynchronize" not in unit and "atomic" not in unit.lower()
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    assert "demc_pointwise.cpp" in makefile and "Fourteen translation units" in makefile
    # the public header: two prototypes, bound by name in the Python binding, none of them in demc.h
    import demc_amd
    public = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "demc_pointwise.h")).read(), flags=re.S)
    protos = sorted(set(re.findall(r"\b(demc_[a-z_0-9]+)\s*\(", public)))
    assert protos == sorted(demc_amd._ffi.PW_EXPORTS) == ["demc_pointwise_loglik", "demc_waic"]
    core = open(os.path.join(ROOT, "include", "demc.h")).read()
    assert "demc_waic" not in core and "demc_pointwise_loglik" not in core
    subprocess.check_call(["gcc", "-std=c99", "-fsyntax-only", "-x", "c", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "include", "demc_pointwise.h")])
    assert (demc_amd._ffi.WAIC_NTOTAL, demc_amd._ffi.WAIC_NPOINT) == (len(demc_amd.chains.WAIC_TOTALS), len(demc_amd.chains.WAIC_POINT)) == (8, 4)


def test_python_restatement_is_the_plan():
    c = plans(["const"])[0]
    assert (c["kPwWG"], c["kPwMinChunk"], c["kPwTargetWG"], c["kPwMaxChunks"], c["kPwPartial"], c["kPwMaxCells"]) == \
        (PW_WG, PW_MIN_CHUNK, PW_TARGET_WG, PW_MAX_CHUNKS, PW_PARTIAL, PW_MAX_CELLS)
    import demc_amd
    assert demc_amd._ffi.PW_MAX_CELLS == PW_MAX_CELLS and (c["DEMC_WAIC_NTOTAL"], c["DEMC_WAIC_NPOINT"]) == (8, 4)
    shapes = sorted({(N, S) for N in (1, 2, 63, 64, 65, 130, 255, 256, 257, 300, 513, 50000, 100000, 600000)
                     for S in (1, 3, 24, 63, 64, 65, 127, 128, 129, 130, 200, 1000, 4097, 409600, 1 << 20)})
    for (N, S), p in zip(shapes, plans([request(1, "lba", N, S, 6, n_acc=3) for N, S in shapes])):
        g = geometry(N, S)
        assert (g["tiles"], g["chunks"], g["chunk_len"]) == (p["tiles"], p["chunks"], p["chunk_len"]), (N, S, g, p)
        assert p["K"] == constants_per_draw("lba", 3) and p["n_part"] == g["chunks"] * PW_PARTIAL * N and p["n_cst"] == S * p["K"]
        assert 1 <= g["last_chunk"] <= g["chunk_len"]
    fams = [("gaussian", {}), ("binomial", {}), ("lnr", dict(n_acc=2)), ("lba", dict(n_acc=8)), ("mvn_iso", dict(direct=True, d=31, dp=32)),
            ("mvn_full", dict(direct=True, d=2, dp=8))]
    for (fam, kw), p in zip(fams, plans([request(0, fam, 65, 70, 3, **kw) for fam, kw in fams])):
        assert p["refused"] == 0 and p["K"] == constants_per_draw(fam, kw.get("n_acc", 0), kw.get("dp", 0)), (fam, p)
        assert p["n_matrix"] == 65 * 70 and p["n_theta"] == 70 * 3 and p["n_part"] == 0
    # the refusals reach the caller through the plan, with their texts
    refused = plans([request(1, "mvn_full", 65, 70, 8, d=8, dp=0), request(0, "hier_gaussian", 65, 70, 8), request(0, "gaussian", 100000, 1343, 2),
                     request(0, "gaussian", 10, 0, 2), request(1, "sim", 10, 5, 2), request(1, "lba", 0, 12, 6, n_acc=3), request(0, "lnr", 0, 12, 4, n_acc=3)])
    assert [r["refused"] for r in refused] == [5, 5, 1, 1, 5, 1, 1]
    assert refused[5]["message"] == "demc_waic: the model holds no observations (N < 1)"
    assert refused[6]["message"] == "demc_pointwise_loglik: the model holds no observations (N < 1)"
    assert "loglike_mode = direct" in refused[0]["message"] and "DEMC_FAM_HIER_GAUSSIAN" in refused[1]["message"]
    assert "above the cap of 134217728 cells" in refused[2]["message"] and refused[3]["message"] == "demc_pointwise_loglik: n < 1"
    assert "simulation likelihood" in refused[4]["message"]


# ---- the header of the two entry points, held to the library and to both bindings as test_cov_host.py holds demc_cov.h
def _pw_prototypes():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "demc_pointwise.h")).read(), flags=re.S)
    protos = {}
    for ret, name, args in re.findall(r"((?:const\s+)?[a-z_0-9]+\s*\**)\s*\b(demc_[a-z_0-9]+)\s*\(([^;{}]*?)\)\s*;", text):
        protos[name] = (ret.strip(), [re.match(r"(.*?[\s\*])([A-Za-z_0-9]+)$", a.strip()).group(1).strip() for a in args.split(",")])
    return text, protos


def test_header_library_and_python_binding_agree():
    import ctypes as C
    import demc_amd
    text, protos = _pw_prototypes()
    assert sorted(protos) == sorted(demc_amd._ffi.PW_EXPORTS)
    for other in (demc_amd._ffi.EXPORTS, demc_amd._ffi.SUMMARY_EXPORTS, demc_amd._ffi.QUANTILE_EXPORTS, demc_amd._ffi.COV_EXPORTS):
        assert not set(protos) & set(other), "declared in another header as well"
    lib = demc_amd._ffi.load()
    ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64, "double*": C.POINTER(C.c_double), "constdouble*": C.POINTER(C.c_double), "demc_handle*": C.c_void_p}
    for name, (ret, args) in protos.items():
        fn = getattr(lib, name)
        assert fn.restype is ctype[ret]
        assert list(fn.argtypes) == [ctype[a.replace(" ", "")] for a in args], (name, args)
    assert len(protos["demc_pointwise_loglik"][1]) == 4 and len(protos["demc_waic"][1]) == 5
    assert "#define DEMC_WAIC_NTOTAL 8" in text and "#define DEMC_WAIC_NPOINT 4" in text and "#define DEMC_PW_MAX_CELLS 134217728" in text
    assert callable(getattr(demc_amd._ffi.HipEngine, "waic")) and callable(getattr(demc_amd._ffi.HipEngine, "pointwise_loglik"))
    assert '#include "demc.h"' in text and "demc_cov.h" not in text and "demc_summary.h" not in text


def test_julia_ccalls_match_their_prototypes():
    import test_julia_shim as J
    _, protos = _pw_prototypes()
    main_jl = open(os.path.join(ROOT, "julia", "DEMCHIP.jl")).read()
    assert 'include("DEMCHIPPointwise.jl")' in main_jl and "demc_waic" not in main_jl and "demc_pointwise_loglik" not in main_jl
    jl = open(os.path.join(ROOT, "julia", "DEMCHIPPointwise.jl")).read()
    calls = list(re.finditer(r"@ccall LIB\.(demc_[a-z_0-9]+)\(", jl))
    assert {m.group(1) for m in calls} >= {"demc_waic", "demc_pointwise_loglik"}
    main = J.c_prototypes()
    for m in calls:
        end = J.balanced(jl, m.end() - 1)
        jtypes = [a[a.rindex("::") + 2:].strip() for a in J.split_top(jl[m.end():end - 1])]
        if m.group(1) in protos:
            cret, ctypes_ = protos[m.group(1)]
            assert jtypes == [J.julia_type(c) for c in ctypes_], (jtypes, ctypes_)
            assert re.match(r"::([A-Za-z0-9{}]+)", jl[end:]).group(1) == J.julia_type(cret)
        else:  # the calls of this file into demc.h itself, against demc.h
            assert m.group(1) in main, m.group(1)
            assert jtypes == [J.julia_type(c) for c in main[m.group(1)][1]], (m.group(1), jtypes)
    import demc_amd
    names = re.search(r"const WAIC_TOTALS = \(([^)]*)\)", jl).group(1)
    assert tuple(n.strip().lstrip(":") for n in names.split(",")) == demc_amd.chains.WAIC_TOTALS


def test_pointwise_kernels_use_no_scratch(tmp_path):
    """the k_pw_* kernels keep everything in registers and LDS, within the registers their workgroups can be given"""
    import pytest
    import demc_amd
    from test_abi import kernel_descriptors
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang-offload-bundler"):
        pytest.skip("no ROCm LLVM tools")
    ks = [k for k in kernel_descriptors(demc_amd._ffi.LIB_PATH, str(tmp_path)) if "k_pw_" in k[0]]
    assert len(ks) == 3 + 2 * 14, [k[0] for k in ks]  # prepare, final, totals; accumulate and matrix for each of the 14 instances
    assert sum("k_pw_accumulate" in k[0] for k in ks) == 14 and sum("k_pw_matrix" in k[0] for k in ks) == 14
    for name, regs, _, wg, scratch in ks:
        assert scratch == 0 and regs <= 512 // -(-wg // 256), (name, regs, wg, scratch)
