"""Compares two `-Rpass-analysis=kernel-resource-usage` reports of the same .hip file (hipcc's stderr) kernel by kernel.

Names are demangled and normalised: the parameter list goes (new kernel parameters change it), and template switches
added at their defaults are dropped — the key-value switches of clo_radix4_pair_kernel (", 0, 0>") and the load type
of clo_radixw_tilehist_kernel when it is the element type. A kernel of the first report is then "identical" when its
registers, scratch, occupancy and LDS are the same in the second. Prints one summary line and every kernel that
changed, went missing or is new.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 ... -Rpass-analysis=kernel-resource-usage -c X.hip -o /dev/null 2> before.txt
    (the same on the other tree) 2> after.txt
    python tools/resource_usage_diff.py before.txt after.txt
"""
import re
import subprocess
import sys


def parse(path):
    recs = {}
    cur = None
    for line in open(path):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            recs[cur] = []
            continue
        m = re.search(r"remark:\s+(.+?) \[-Rpass", line)
        if m and cur:
            recs[cur].append(m.group(1))
    names = list(recs)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    out = {}
    for n, d in zip(names, dem):
        d = d.replace("(anonymous namespace)::", "")
        i = d.find(">(")
        d = d[:i + 1] if i >= 0 else re.sub(r"\(.*\)$", "", d)   # parameter list
        d = re.sub(r", 0, 0>$", ">", d) if "pair_kernel" in d else d   # the new switches at their defaults
        d = re.sub(r", unsigned long>$", ">", d) if ("tilehist_kernel<unsigned long," in d) else d
        m = re.match(r"(.*tilehist_kernel<(unsigned \w+|unsigned long), .*), (unsigned \w+|unsigned long)>$", d)
        if m and m.group(2) == m.group(3):
            d = m.group(1) + ">"
        out[d] = recs[n]
    return out


a, b = parse(sys.argv[1]), parse(sys.argv[2])
same = [k for k in a if k in b and a[k] == b[k]]
diff = [k for k in a if k in b and a[k] != b[k]]
gone = [k for k in a if k not in b]
new = [k for k in b if k not in a]
print("%s: %d kernels before, %d after: %d identical, %d differ, %d missing, %d new" % (sys.argv[1].split('/')[-1], len(a), len(b), len(same), len(diff), len(gone), len(new)))
for k in diff + gone:
    print("  CHANGED/MISSING", k)
for k in new:
    print("  NEW", k, "|", "; ".join(x for x in b[k] if x.split(":")[0] in ("VGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]", "TotalSGPRs")))
