#!/usr/bin/env python3
"""Does a change to the NLP iteration (etol_amd/host/emi_nlp.cpp) leave every solve as it was, bit for bit?  Run in two trees -- the
parent commit's and the changed one, each with its own built libraries -- and compare what they write:

   python tools/nlp_identity.py cpu OUT.json       the solves of tests/test_host_cpu.py (oracle evaluator, no device)
   python tools/nlp_identity.py gpu OUT.json       small solves of tests/test_gpu_solve.py / test_gpu_delays.py through eMI355X
   python tools/nlp_identity.py strategy OUT.json  the mesh strategy's own paths (host/emi_mesh_driver.cpp): Monte-Carlo scenario sets whose solves
                                                  restart the ladder, through etol_mi355x_montecarlo, one child process per set
   python tools/nlp_identity.py compare PARENT.json BRANCH.json [OUT.json]      equal or not, field by field (times are reported only)
   python tools/nlp_identity.py cpu-times LABEL OUT.jsonl      one more wall time per cpu case, appended as a line: run it in the two
                                                               trees in turn, round after round, so that both see the same machine
   python tools/nlp_identity.py compare-times OUT.jsonl        best time per case and tree; the branch may exceed the parent by the
                                                               parent's own spread

Per case: SHA-256 of the bytes of the trajectory and the cost, iteration count, return code and message, and SHA-256 of the solve's
stdout at print_level 6 (the per-iteration trace; the timing summary lines are cut out).  `cpu` adds three wall times of the call at
print_level 0, `gpu` adds Sol::nlp_runs (nodes, iterations, converged).  `strategy` records per scenario the return code, nodes,
iterations, the printed cost, the runs list and the SHA-256 of the strategy's own printed lines, and the wall time of each child.  The libraries are those of the tree the script lies in."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
ORACLE = os.path.join(ROOT, "oracle", "liboracle.so").encode()
D, I = C.POINTER(C.c_double), C.POINTER(C.c_int)
libc = C.CDLL(None)


def harness():
    import torch  # noqa: F401  (one HIP runtime per process: see etol_amd/_lib.py)
    H = C.CDLL(os.path.join(ROOT, "tests", "harness", "libetol_harness.so"))
    H.harness_last_message.restype = C.c_char_p
    H.harness_set_linear_solver.argtypes = [C.c_char_p]
    H.harness_set_node_blocks.argtypes = [C.c_char_p]
    H.harness_set_scaling.argtypes = [C.c_int]
    H.harness_last_nlp_runs.argtypes = [D, C.c_int]
    H.harness_solve_example1_oracle.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_double, C.c_int, C.c_int, D, I, D, D, C.c_int, I]
    H.harness_solve_quadrotor_oracle.argtypes = [C.c_char_p, C.c_int, C.c_double, C.c_int, C.c_double, C.c_int, D, I, D, D, C.c_int, I]
    H.harness_solve_fixedwing_oracle.argtypes = [C.c_char_p, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int, D, I, D, D, C.c_int, I]
    H.harness_solve_delay_demo_oracle.argtypes = [C.c_char_p, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, D, D, I]
    H.harness_solve_example1.argtypes = [C.c_char_p, C.c_int, C.c_double, C.c_int, D, I, D, D, D, C.c_int, I]
    H.harness_solve_quadrotor.argtypes = [C.c_int, C.c_double, C.c_int, C.c_double, C.c_int, C.c_int, C.c_double, D, I, D, D, C.c_int, I, I, D]
    H.harness_solve_fixedwing.argtypes = [C.c_int, C.c_double, C.c_double, C.c_double, C.c_int, D, I, D, D, C.c_int, I]
    H.harness_solve_delay_demo.argtypes = [C.c_int, C.c_double, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, D, D, D, I, D]
    return H


def captured(call):
    """stdout of call(), taken at file-descriptor level (the solver prints through C stdio)"""
    sys.stdout.flush()
    libc.fflush(None)
    keep = os.dup(1)
    with tempfile.TemporaryFile() as f:
        os.dup2(f.fileno(), 1)
        try:
            out = call()
            libc.fflush(None)
        finally:
            os.dup2(keep, 1)
            os.close(keep)
        f.seek(0)
        return out, f.read()


def sha(b):
    return hashlib.sha256(b).hexdigest()


def run(H, fn, args, print_at, arrays):
    """one harness solve: args[print_at] is its print_level; arrays = (X, U) or (Z,); the last argument is the iteration count"""
    cost, it = C.c_double(), C.c_int()
    bufs = [np.zeros(n) for n in arrays]

    def call(level):
        named = dict(cost=C.byref(cost), iters=C.byref(it), **{f"buf{i}": b.ctypes.data_as(D) for i, b in enumerate(bufs)})
        a = [named[x] if isinstance(x, str) else x for x in args]
        a[print_at] = level
        for b in bufs:
            b[:] = 0
        return fn(*a)

    rc, text = captured(lambda: call(6))
    trace = b"\n".join(ln for ln in text.split(b"\n") if not ln.startswith(b"time: total"))
    rec = dict(rc=rc, message=H.harness_last_message().decode() if rc else "", iterations=it.value, cost=sha(bytes(cost)),
               trace=sha(trace), trace_lines=trace.count(b"\n"), **{f"array{i}": sha(b.tobytes()) for i, b in enumerate(bufs)})
    return rec, call


def cpu_cases(H, xml):
    M = C.c_int()
    for wo in (0, 1):
        yield f"example1 oracle obstacles={wo}", H.harness_solve_example1_oracle, \
            [xml, ORACLE, wo, 1e-9, 0, 400, "cost", C.byref(M), "buf0", "buf1", 64, "iters"], 4, (128, 128), True
    yield "quadrotor oracle", H.harness_solve_quadrotor_oracle, [ORACLE, 24, 0.16, 2, 1e-8, 0, "cost", C.byref(M), "buf0", "buf1", 64, "iters"], \
        5, (6 * 64, 2 * 64), True
    yield "fixedwing oracle", H.harness_solve_fixedwing_oracle, [ORACLE, 24, 8.0, 10.0, 1e-7, 0, "cost", C.byref(M), "buf0", "buf1", 32, "iters"], \
        5, (12 * 32, 4 * 32), True
    for disc_r, scaling in ((0.9, 0), (0.9, 1), (0.5, 1), (0.0, 0)):        # coupling rows: the dense backend only
        yield f"delay demo oracle disc_r={disc_r} scaling={scaling}", H.harness_solve_delay_demo_oracle, \
            [ORACLE, 24, 0.25, disc_r, 1e-10, 0, scaling, "cost", "buf0", "iters"], 5, (10 * 25,), False


def cpu_times(H, xml):
    out = {}
    for name, fn, args, print_at, arrays, variants in cpu_cases(H, xml):
        for solver in (b"auto", b"device") if variants else (b"auto",):
            for scaling in (0, 1) if variants else (-1,):
                H.harness_set_linear_solver(solver)
                H.harness_set_scaling(scaling)
                cost, it = C.c_double(), C.c_int()
                bufs = [np.zeros(n) for n in arrays]
                named = dict(cost=C.byref(cost), iters=C.byref(it), **{f"buf{i}": b.ctypes.data_as(D) for i, b in enumerate(bufs)})
                t0 = time.perf_counter()
                fn(*[named[x] if isinstance(x, str) else x for x in args])
                out[name + (f" linear_solver={solver.decode()} scaling={scaling}" if variants else "")] = time.perf_counter() - t0
    return out


def compare_times(path):
    runs = [json.loads(ln) for ln in open(path)]
    rep, slower = {}, []
    for case in runs[0]["seconds"]:
        t = {lab: [r["seconds"][case] for r in runs if r["label"] == lab] for lab in ("parent", "branch")}
        spread = max(t["parent"]) - min(t["parent"])
        rep[case] = dict(parent_best=min(t["parent"]), branch_best=min(t["branch"]), parent_spread=spread,
                         within_parent_spread=min(t["branch"]) - min(t["parent"]) <= spread)
        if not rep[case]["within_parent_spread"]:
            slower.append(case)
    return rep, slower


def cpu(H, xml):
    out = {}
    for name, fn, args, print_at, arrays, variants in cpu_cases(H, xml):
        for solver in (b"auto", b"device") if variants else (b"auto",):
            for scaling in (0, 1) if variants else (-1,):
                H.harness_set_linear_solver(solver)
                H.harness_set_scaling(scaling)
                rec, call = run(H, fn, args, print_at, arrays)
                rec["seconds"] = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    call(0)
                    rec["seconds"].append(time.perf_counter() - t0)
                key = name + (f" linear_solver={solver.decode()} scaling={scaling}" if variants else "")
                out[key] = rec
                print(f"{min(rec['seconds']):8.3f} s  rc={rec['rc']} it={rec['iterations']:4d} trace {rec['trace'][:12]} ({rec['trace_lines']} lines)  {key}",
                      flush=True)
    H.harness_set_linear_solver(b"auto")
    H.harness_set_scaling(-1)
    return out


def gpu_cases(H, xml):
    M, mit, oerr, dmax = C.c_int(), C.c_int(), C.c_double(), C.c_double()
    T = np.zeros(160)
    yield "example1 with keep-outs", H.harness_solve_example1, \
        [xml, 1, 1e-9, 0, "cost", C.byref(M), "buf0", "buf1", T.ctypes.data_as(D), 160, "iters"], 3, (2 * 160, 2 * 160), True
    yield "quadrotor 41 nodes", H.harness_solve_quadrotor, \
        [40, 0.1, 2, 1e-10, 0, 0, 1e-4, "cost", C.byref(M), "buf0", "buf1", 160, "iters", C.byref(mit), C.byref(oerr)], 4, (6 * 160, 2 * 160), True
    yield "fixedwing 129 nodes", H.harness_solve_fixedwing, [128, 12.0, 20.0, 1e-7, 0, "cost", C.byref(M), "buf0", "buf1", 129, "iters"], \
        4, (12 * 129, 4 * 129), True
    for nsteps, disc_r in ((24, 0.9), (32, 0.5), (40, 0.0)):               # coupling rows: the dense backend only
        yield f"delay demo nsteps={nsteps} disc_r={disc_r}", H.harness_solve_delay_demo, \
            [nsteps, 0.25, 3, 1, disc_r, 1e-10, 0, "cost", "buf0", "buf1", "iters", C.byref(dmax)], 6, (2 * (nsteps + 1), 2 * (nsteps + 1)), False


def gpu(H, xml):
    out = {}
    runs = np.zeros(12 * 64)
    for name, fn, args, print_at, arrays, variants in gpu_cases(H, xml):
        for solver, blocks in ((b"host", b"host"), (b"device", b"host"), (b"device", b"device")) if variants else ((b"auto", b"host"),):
            H.harness_set_linear_solver(solver)
            H.harness_set_node_blocks(blocks)
            rec, _ = run(H, fn, args, print_at, arrays)
            n = H.harness_last_nlp_runs(runs.ctypes.data_as(D), runs.size)
            rec["nlp_runs"] = [[int(v) for v in runs[i:i + 3]] for i in range(0, min(n, runs.size), 12)]
            key = name + (f" linear_solver={solver.decode()} node_blocks={blocks.decode()}" if variants else "")
            out[key] = rec
            print(f"rc={rec['rc']} it={rec['iterations']:4d} runs {rec['nlp_runs']} trace {rec['trace'][:12]} ({rec['trace_lines']} lines)  {key}", flush=True)
            if rec["rc"] != 0:          # nothing further after a solve that did not end well
                json.dump(out, open(sys.argv[2], "w"), indent=1, sort_keys=True)
                sys.exit(f"{key}: rc {rec['rc']} {rec['message']}")
    H.harness_set_linear_solver(b"auto")
    H.harness_set_node_blocks(b"")
    return out


# (arguments of etol_mi355x_montecarlo, extra environment, time limit of the child in seconds): the sets tests/test_gpu_solve.py uses,
# and scenario 27 again with the straight line as the first start of a climb (EMI_MC_PLAN=1: the planned route second, 0: last) -- since
# the planned route became the first start it climbs straight through, and with the line first its ladder fails and restarts
STRATEGY_SETS = ((("10", "128", "8", "1"), {}, 300), (("32", "256", "10", "1"), {"EMI_MC_ONLY": "27"}, 300),
                 (("32", "512", "20", "1"), {"EMI_MC_ONLY": "27"}, 300), (("32", "256", "10", "1"), {"EMI_MC_ONLY": "27", "EMI_MC_PLAN": "0"}, 300),
                 (("32", "512", "20", "1"), {"EMI_MC_ONLY": "27", "EMI_MC_PLAN": "1"}, 300), (("32", "512", "20", "1"), {"EMI_MC_ONLY": "27", "EMI_MC_PLAN": "0"}, 300))
STRATEGY_LINES = ("mesh sequencing:", "cold start", "warm start", "mesh iteration")


def strategy():
    exe = os.path.join(ROOT, "etol_amd", "lib", "etol_mi355x_montecarlo")
    out = {}
    for args, extra, limit in STRATEGY_SETS:
        env = dict(os.environ, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", EMI_MC_RUNS="1", EMI_MC_PRINT_LEVEL="5", EMI_MC_GATHER="0", **extra)
        name = "montecarlo " + " ".join(args) + "".join(f" {k}={v}" for k, v in extra.items())
        t0 = time.perf_counter()
        r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=limit, env=env)
        seconds = time.perf_counter() - t0
        if r.returncode not in (0, 2):          # (2: not every scenario solved)
            json.dump(out, open(sys.argv[2], "w"), indent=1, sort_keys=True)
            sys.exit(f"{name}: exit status {r.returncode}\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
        lines = r.stdout.split("\n")
        printed = "\n".join(ln for ln in lines if ln.startswith(STRATEGY_LINES))
        scenarios = {}
        for ln in lines:
            f = ln.split()
            if ln.startswith("scenario") and "runs" in f:
                scenarios[f[1]] = dict(rc=int(f[f.index("rc") + 1]), nodes=int(f[f.index("nodes") + 1]), iterations=int(f[f.index("iterations") + 1]),
                                       cost=f[f.index("cost") + 1], runs=f[f.index("runs") + 1:])
        out[name] = dict(exit_status=r.returncode, scenarios=scenarios, strategy_lines=sha(printed.encode()),
                         strategy_line_count=printed.count("\n") + 1 if printed else 0, seconds=[seconds])
        print(f"{seconds:8.2f} s  exit {r.returncode}  {len(scenarios)} scenarios  strategy lines {out[name]['strategy_lines'][:12]} "
              f"({out[name]['strategy_line_count']})  {name}", flush=True)
    return out


def compare(pa, br):
    report = dict(equal=[], different={}, seconds={})
    for name in sorted(set(pa) | set(br)):
        a, b = pa.get(name, {}), br.get(name, {})
        diff = [k for k in sorted(set(a) | set(b)) if k != "seconds" and a.get(k) != b.get(k)]
        if name not in pa or name not in br:
            diff = ["case missing in the " + ("parent's" if name not in pa else "branch's") + " record"]
        if diff:
            report["different"][name] = diff
        else:
            report["equal"].append(name)
        if "seconds" in a and "seconds" in b:
            report["seconds"][name] = dict(parent=a["seconds"], branch=b["seconds"], parent_best=min(a["seconds"]), branch_best=min(b["seconds"]),
                                           parent_spread=max(a["seconds"]) - min(a["seconds"]),
                                           within_parent_spread=min(b["seconds"]) - min(a["seconds"]) <= max(a["seconds"]) - min(a["seconds"]))
    report["verdict"] = "identical" if not report["different"] and report["equal"] else "DIFFERENT"
    return report


if __name__ == "__main__":
    mode = sys.argv[1]
    if mode == "compare":
        pa, br = (json.load(open(f)) for f in sys.argv[2:4])
        rep = compare(pa, br)
        print(json.dumps(dict(verdict=rep["verdict"], equal=len(rep["equal"]), different=rep["different"],
                              slower_than_parent_spread=[k for k, v in rep["seconds"].items() if not v["within_parent_spread"]])))
        if len(sys.argv) > 4:
            json.dump(dict(rep, parent=pa, branch=br), open(sys.argv[4], "w"), indent=1, sort_keys=True)
        sys.exit(0 if rep["verdict"] == "identical" else 1)
    if mode == "compare-times":
        rep, slower = compare_times(sys.argv[2])
        for case, r in rep.items():
            print(f"{r['parent_best']:9.4f} s parent  {r['branch_best']:9.4f} s branch  spread {r['parent_spread']:.4f}  {'ok    ' if r['within_parent_spread'] else 'SLOWER'}  {case}")
        sys.exit(1 if slower else 0)
    import gen_xml_fixtures as G
    xml = G.write_all(tempfile.mkdtemp())["ocp_2d_ex1.xml"].encode()
    if mode == "cpu-times":
        with open(sys.argv[3], "a") as f:
            f.write(json.dumps(dict(label=sys.argv[2], seconds=cpu_times(harness(), xml))) + "\n")
        sys.exit(0)
    res = strategy() if mode == "strategy" else (cpu if mode == "cpu" else gpu)(harness(), xml)
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
    json.dump(res, open(sys.argv[2], "w"), indent=1, sort_keys=True)
    print(mode, len(res), "cases ->", sys.argv[2], sha(json.dumps({k: {f: v for f, v in r.items() if f != "seconds"} for k, r in res.items()},
                                                                    sort_keys=True).encode())[:16])
