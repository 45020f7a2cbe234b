#!/usr/bin/env python3
"""Per-kernel register and occupancy table from the compiler's resource remarks, one build against another.

Build the library twice (parent and change) with the remarks switched on and the compiler's stderr kept:

    make -C sourmash_amd/csrc -j8 -Otarget CXXFLAGS="-O3 -std=c++17 -fPIC -fvisibility=hidden -Wall -Wno-unused-function \\
        -Rpass-analysis=kernel-resource-usage" 2> build.log

(-Otarget: one compiler's remarks must not be cut into by another's, the fields of a kernel follow its name line by line)

then: python tools/kernel_resources.py before.log after.log [-o profiles/NAME.txt]

Every kernel of every translation unit is compared, matched by its name demangled with c++filt and without its argument list.  The table lists the kernels
whose VGPR count, occupancy, scratch, spill counts or LDS size differ, then a summary; the exit status is 1 when any kernel lost a
wave per SIMD, gained scratch, gained a spill or changed its LDS size."""
import re
import shutil
import subprocess
import sys

FIELDS = {"VGPRs": "vgpr", "AGPRs": "agpr", "ScratchSize [bytes/lane]": "scratch", "Occupancy [waves/SIMD]": "occ",
          "SGPRs Spill": "sspill", "VGPRs Spill": "vspill", "LDS Size [bytes/block]": "lds", "TotalSGPRs": "sgpr"}


def parse(path):
    out, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark:\s+(.*?)\s*\[-Rpass-analysis", line)
        if not m:
            continue
        t = re.sub(r"^\S+:\d+:\d+:\s+", "", m.group(1))     # "remark: file:line:col: text" as well as "file:line:col: remark: text"
        if t.startswith("Function Name:"):
            cur = out.setdefault(t.split(":", 1)[1].strip(), {})
        elif cur is not None and ":" in t:
            k, v = t.rsplit(":", 1)
            if k.strip() in FIELDS:
                cur[FIELDS[k.strip()]] = int(v)
    return out


def strip_args(d):
    "drop the return type and the closing argument list of a demangled kernel name"
    d = d.replace("void ", "", 1) if d.startswith("void ") else d
    if not d.endswith(")"):
        return d
    depth = 0
    for i in range(len(d) - 1, -1, -1):
        depth += (d[i] == ")") - (d[i] == "(")
        if depth == 0:
            return d[:i]
    return d


def demangle(names):
    if not shutil.which("c++filt"):
        return {n: n for n in names}
    res = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    return {n: strip_args(r) for n, r in zip(names, res)}


def main():
    args = [a for a in sys.argv[1:] if a != "-o"]
    dest = sys.argv[sys.argv.index("-o") + 1] if "-o" in sys.argv else None
    if dest:
        args.remove(dest)
    before, after = parse(args[0]), parse(args[1])
    # matched by the demangled name without its argument list: a kernel that gains an argument is still the same kernel
    nice = demangle(sorted(set(before) | set(after)))
    before, after = {nice[n]: v for n, v in before.items()}, {nice[n]: v for n, v in after.items()}
    names = sorted(set(before) | set(after))
    nice = {n: n for n in names}
    rows, worse, missing = [], [], []
    for n in names:
        b, a = before.get(n), after.get(n)
        if b is None or a is None:
            missing.append(nice[n] + (" (only after)" if b is None else " (only before)"))
            continue
        if a["occ"] < b["occ"] or a["scratch"] > b["scratch"] or a["vspill"] > b["vspill"] or a["sspill"] > b["sspill"] or a["lds"] != b["lds"]:
            worse.append(nice[n])
        if any(a[k] != b[k] for k in ("vgpr", "agpr", "occ", "scratch", "vspill", "sspill", "lds")):
            rows.append((nice[n], b, a))
    lines = [f"kernels compared: {len(names) - len(missing)}; VGPR / occupancy / scratch / spill / LDS differ in {len(rows)}; "
             f"lost a wave per SIMD, gained scratch, gained a spill or changed LDS: {len(worse)}",
             f"kernels with scratch: before {sum(1 for v in before.values() if v['scratch'])}, after {sum(1 for v in after.values() if v['scratch'])}; "
             f"with spills: before {sum(1 for v in before.values() if v['vspill'] or v['sspill'])}, "
             f"after {sum(1 for v in after.values() if v['vspill'] or v['sspill'])}", ""]
    lines.append(f"{'kernel':<64} {'VGPR':>9} {'occ':>5} {'scratch':>9} {'v-spill':>8} {'s-spill':>8} {'LDS':>13}")
    for name, b, a in rows:
        lines.append(f"{name:<64} {b['vgpr']:>4}>{a['vgpr']:<4} {b['occ']}>{a['occ']:<3} {b['scratch']:>4}>{a['scratch']:<4} "
                     f"{b['vspill']:>3}>{a['vspill']:<4} {b['sspill']:>3}>{a['sspill']:<4} {b['lds']:>6}>{a['lds']:<6}")
    lines += [""] + [f"WORSE: {w}" for w in worse] + [f"UNMATCHED: {m}" for m in missing]
    text = "\n".join(lines).rstrip() + "\n"
    if dest:
        open(dest, "w").write(text)
    sys.stdout.write(text)
    sys.exit(1 if worse else 0)


if __name__ == "__main__":
    main()
