"""Static comparison of the gfx950 kernels inside two object files (no GPU): for a change that must leave device code as it is
where the bytes cannot stay the same.

    python tools/codeobj_diff.py OLD.o NEW.o KERNEL_SUBSTRING LABEL [--all]

Both objects are unbundled the way profiles/linear_plan.txt describes (llvm-objcopy --only-section=.hip_fatbin, clang-offload-bundler
--unbundle of the hipv4-...gfx950 entry).  Per kernel whose demangled name contains KERNEL_SUBSTRING, from the metadata note
(llvm-readelf --notes) and llvm-objdump -d:
  (a) resources: VGPR / AGPR / SGPR counts, private segment size, VGPR / SGPR spill counts, static LDS, code size;
  (b) synchronisation skeleton: the ordered subsequence of barriers, wait-counter instructions (with their immediates) and LDS-DMA
      loads, with the number of matrix instructions between consecutive entries; register numbers play no part;
  (c) the difference of the per-mnemonic instruction histograms.
A line per kernel (details only where something differs, or with --all), then a summary line that starts with LABEL.  Exit status 1
when a kernel is missing on one side or differs in (a) -- code size apart -- or in (b)."""
import collections
import os
import re
import shutil
import subprocess
import sys
import tempfile

TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
RESOURCES = (("vgpr", ".vgpr_count"), ("agpr", ".agpr_count"), ("sgpr", ".sgpr_count"), ("private", ".private_segment_fixed_size"),
             ("vgpr_spill", ".vgpr_spill_count"), ("sgpr_spill", ".sgpr_spill_count"), ("lds", ".group_segment_fixed_size"))


def llvm(tool):
    for d in (os.environ.get("LLVM_BIN"), "/opt/rocm/lib/llvm/bin", "/opt/rocm/llvm/bin"):
        if d and os.path.exists(os.path.join(d, tool)):
            return os.path.join(d, tool)
    found = shutil.which(tool)
    if not found:
        raise RuntimeError("%s not found (set LLVM_BIN)" % tool)
    return found


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def kernels(obj, tmp, tag):
    """{mangled name: dict(res={...}, insts=[(mnemonic, operands)], size=bytes)} of the gfx950 code object in obj"""
    fat, co = os.path.join(tmp, tag + ".fatbin"), os.path.join(tmp, tag + ".co")
    run(llvm("llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", obj, fat)
    run(llvm("clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat, "--targets=" + TARGET, "--output=" + co)
    out, cur = {}, None
    for line in run(llvm("llvm-readelf"), "--notes", co).splitlines():
        m = re.match(r"\s*(?:- )?(\.\w+):\s+(\S+)\s*$", line)
        if not m:
            continue
        if line.lstrip().startswith("- .") and m.group(1) in (".agpr_count", ".args"):
            cur = {}                                                    # a new entry of amdhsa.kernels
        if cur is None:
            continue
        cur[m.group(1)] = m.group(2)
        if m.group(1) == ".wavefront_size":                             # the entry's last key
            out[cur[".name"]] = dict(res={k: int(cur[f]) for k, f in RESOURCES}, insts=[], size=0)
            cur = None
    name = None
    for line in run(llvm("llvm-objdump"), "-d", co).splitlines():
        m = re.match(r"[0-9a-f]+ <(.+)>:$", line)
        if m:
            name = m.group(1) if m.group(1) in out else None
            continue
        m = re.match(r"\s+(\S+)\s*(.*?)\s*// [0-9A-F]+: ((?:[0-9A-F]{8} ?)+)$", line)
        if name and m:
            out[name]["insts"].append((m.group(1), m.group(2)))
            out[name]["size"] += 4 * len(m.group(3).split())
    return out


def skeleton(insts):
    """[(kind, text, matrix instructions since the previous entry)], and the matrix instructions behind the last one"""
    sk, n = [], 0
    for mn, ops in insts:
        if "mfma" in mn:
            n += 1
        elif "barrier" in mn:
            sk.append(("barrier", mn, n)); n = 0
        elif mn.startswith("s_wait"):
            sk.append(("wait", mn + " " + ops, n)); n = 0
        elif "load" in mn and (re.search(r"\blds\b", ops) or "_lds_" in mn):
            sk.append(("lds-dma", mn, n)); n = 0
    return sk, n


def main():
    args = [a for a in sys.argv[1:] if a != "--all"]
    if len(args) != 4:
        sys.exit(__doc__)
    old_o, new_o, sub, label = args
    show_all = "--all" in sys.argv
    with tempfile.TemporaryDirectory() as tmp:
        old, new = kernels(old_o, tmp, "old"), kernels(new_o, tmp, "new")
    names = sorted(set(old) | set(new))
    filt = next((p for p in (shutil.which("llvm-cxxfilt"), shutil.which("c++filt")) if p), None)      # names stay mangled without one
    pretty = dict(zip(names, run(filt, *names).splitlines())) if filt and names else {n: n for n in names}
    names = [n for n in names if sub in pretty[n]]
    bad_res = bad_sk = missing = 0
    d_insts, hist_all = 0, collections.Counter()
    for n in names:
        if n not in old or n not in new:
            print("%s: only in %s" % (pretty[n], "OLD" if n in old else "NEW"))
            missing += 1
            continue
        a, b = old[n], new[n]
        res_diff = [k for k, _ in RESOURCES if a["res"][k] != b["res"][k]]
        (ska, ta), (skb, tb) = skeleton(a["insts"]), skeleton(b["insts"])
        sk_same = ska == skb and ta == tb
        ha, hb = collections.Counter(m for m, _ in a["insts"]), collections.Counter(m for m, _ in b["insts"])
        hd = {m: hb[m] - ha[m] for m in sorted(set(ha) | set(hb)) if ha[m] != hb[m]}
        bad_res += bool(res_diff)
        bad_sk += not sk_same
        d_insts += len(b["insts"]) - len(a["insts"])
        hist_all.update(hd)
        print("%s: resources %s, skeleton %s (%d entries, %d matrix), code %d -> %d B, instructions %d -> %d"
              % (pretty[n], "DIFFER" if res_diff else "same", "same" if sk_same else "DIFFERS", len(ska), sum(e[2] for e in ska) + ta,
                 a["size"], b["size"], len(a["insts"]), len(b["insts"])))
        if res_diff or show_all:
            print("    " + "  ".join("%s %d%s" % (k, a["res"][k], "" if a["res"][k] == b["res"][k] else " -> %d" % b["res"][k]) for k, _ in RESOURCES))
        if not sk_same:
            i = next((i for i, (x, y) in enumerate(zip(ska, skb)) if x != y), min(len(ska), len(skb)))
            print("    skeleton: %d / %d entries, first difference at %d: %s | %s" % (len(ska), len(skb), i, ska[i:i + 3], skb[i:i + 3]))
        if hd:
            print("    histogram: " + "  ".join("%s %+d" % kv for kv in hd.items()))
    print("%s: %d kernels matching '%s': %d missing on one side, %d differ in resources, %d differ in skeleton, instructions %+d"
          % (label, len(names), sub, missing, bad_res, bad_sk, d_insts))
    if hist_all:
        print("%s: histogram differences over all kernels: %s" % (label, "  ".join("%s %+d" % kv for kv in sorted(hist_all.items()) if kv[1])))
    sys.exit(1 if (missing or bad_res or bad_sk or not names) else 0)


if __name__ == "__main__":
    main()
