#!/usr/bin/env python3
"""The register budget of emi_pass_f64_kernel, checked (`make check-pass-registers`): cross-compile etol_amd/csrc/emi_symdefect.hip for
gfx950 with -Rpass-analysis=kernel-resource-usage (the engine of tools/kres.py) and hold every instantiation to the resident workgroups
per CU it states (its last template argument, RES):
  * RES = 3: occupancy 3 waves per SIMD, VGPRs + AGPRs <= 168 (512 / 3 rounded down to the allocation granule of 8), no scratch.
    amdgpu_waves_per_eu(2, 3) lets the compiler fall back to two waves silently once a source change needs more; this does not.
  * RES = 2: no scratch, and VGPRs, AGPRs and occupancy as recorded in tools/pass_registers.json (--record writes it).  VGPRs are recorded
    and compared as ALLOCATED: the compiler's count rounded up to the allocation granule of 8, which is what a wave takes of the
    register file and what decides how many are resident -- 156 and 160 registers are the same allocation.  (--list prints the raw counts.)
No device needed.   python tools/check_pass_registers.py [--record] [--hipcc PATH] [--arch gfx950] [--list]"""
import argparse
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join("etol_amd", "csrc", "emi_symdefect.hip")
RECORD = os.path.join(ROOT, "tools", "pass_registers.json")
BUDGET_RES3 = 168
GRANULE = 8


def allocated(n):
    """registers a wave is given for a count of n: whole granules"""
    return (n + GRANULE - 1) // GRANULE * GRANULE
KERNEL = "emi_pass_f64_kernel"
ARGS = ("model", "sw", "vec", "st", "nst", "bk", "ct", "hs", "keep", "dop", "res")


def resource_usage(hipcc, arch):
    """[{name (demangled), vgpr, agpr, scratch, occ, lds}] of every kernel of the source"""
    cmd = [hipcc, f"--offload-arch={arch}", "--cuda-device-only", "-O3", "-std=c++17", "-fPIC", "-Iinclude", "-Ietol_amd/csrc", "-c", SOURCE, "-o", os.devnull,
           "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit("compile failed:\n" + r.stderr[-4000:])
    rows, cur = [], None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+([\w \[\]/]+?): (.*?) \[-Rpass", line)
        if not m:
            continue
        k, v = m.group(1).strip(), m.group(2).strip()
        if k in ("Function Name", "Name"):
            cur = {"mangled": v}
            rows.append(cur)
        elif cur is not None:
            cur[k] = v
    names = subprocess.run(["c++filt"], input="\n".join(x["mangled"] for x in rows), capture_output=True, text=True).stdout.splitlines()
    out = []
    for x, name in zip(rows, names):
        out.append(dict(name=name.strip(), vgpr=int(x.get("VGPRs", -1)), agpr=int(x.get("AGPRs", -1)), scratch=int(x.get("ScratchSize [bytes/lane]", -1)),
                        occ=int(x.get("Occupancy [waves/SIMD]", -1)), lds=int(x.get("LDS Size [bytes/block]", -1))))
    return out


def split_args(text):
    """top-level comma split of a template argument list"""
    parts, depth, cur = [], 0, ""
    for ch in text:
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        if ch == "," and depth == 0:
            parts.append(cur.strip())
            cur = ""
        else:
            cur += ch
    parts.append(cur.strip())
    return parts


def pass_instantiations(rows):
    """{key: row} of the instantiations of the pass kernel; key = its template arguments, RES included"""
    out = {}
    for x in rows:
        m = re.search(KERNEL + r"<(.*)>\(", x["name"])
        if not m:
            continue
        args = split_args(m.group(1))
        if len(args) != len(ARGS):
            sys.exit(f"unexpected template arguments: {x['name']}")
        a = dict(zip(ARGS, args))
        a["model"] = re.sub(r"^emi::|<double>$", "", a["model"])
        key = ", ".join(a[k] for k in ARGS)
        out[key] = dict(x, **a)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hipcc", default=os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    ap.add_argument("--arch", default="gfx950")
    ap.add_argument("--record", action="store_true", help="write tools/pass_registers.json from this compile (the RES = 2 instantiations)")
    ap.add_argument("--list", action="store_true", help="print every instantiation")
    a = ap.parse_args()
    inst = pass_instantiations(resource_usage(a.hipcc, a.arch))
    if not inst:
        sys.exit("no instantiation of " + KERNEL + " found")
    if a.list:
        for key, x in sorted(inst.items()):
            print(f"{key:60s} vgpr={x['vgpr']:4d} agpr={x['agpr']:3d} scratch={x['scratch']:4d} occ={x['occ']:2d} lds={x['lds']}")
    two = {k: x for k, x in inst.items() if x["res"] == "2"}
    three = {k: x for k, x in inst.items() if x["res"] == "3"}
    if a.record:
        with open(RECORD, "w") as f:
            json.dump({k: dict(vgpr=allocated(x["vgpr"]), agpr=x["agpr"], occ=x["occ"]) for k, x in sorted(two.items())}, f, indent=0, sort_keys=True)
            f.write("\n")
        print(f"recorded {len(two)} instantiations that state 2 in {os.path.relpath(RECORD, ROOT)}")
    with open(RECORD) as f:
        recorded = json.load(f)
    bad = []
    for key, x in sorted(three.items()):
        if x["dop"] != "true":
            bad.append(f"{key}: states 3 without De / Do from L2")
        if x["occ"] != 3 or x["vgpr"] + x["agpr"] > BUDGET_RES3 or x["scratch"] != 0:
            bad.append(f"{key}: states 3, reports occupancy {x['occ']}, {x['vgpr']} + {x['agpr']} registers (budget {BUDGET_RES3}), scratch {x['scratch']}")
    for key, x in sorted(two.items()):
        if x["scratch"] != 0:
            bad.append(f"{key}: scratch {x['scratch']}")
        want = recorded.get(key)
        if want is None:
            bad.append(f"{key}: not in the record (python tools/check_pass_registers.py --record)")
        elif (allocated(x["vgpr"]), x["agpr"], x["occ"]) != (allocated(want["vgpr"]), want["agpr"], want["occ"]):
            bad.append(f"{key}: reports {x['vgpr']} + {x['agpr']} registers ({allocated(x['vgpr'])} allocated), occupancy {x['occ']}; recorded {want['vgpr']} + {want['agpr']}, "
                       f"occupancy {want['occ']}")
    for key in sorted(set(recorded) - set(two)):
        bad.append(f"{key}: recorded, no longer instantiated")
    # every direct-operator instantiation that states 2 has its twin that states 3
    for key, x in sorted(two.items()):
        if x["dop"] == "true" and key[: key.rfind(",")] + ", 3" not in three:
            bad.append(f"{key}: no instantiation that states 3")
    print(f"pass registers: {len(three)} instantiations state 3, {len(two)} state 2, {len(bad)} failures")
    for b in bad:
        print("  " + b)
    if bad:
        sys.exit(1)
    print("pass registers: ok")


if __name__ == "__main__":
    main()
