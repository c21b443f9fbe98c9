"""Kernel resource usage of two builds of kernels.hip, side by side.

Build each tree's kernels.hip with the Makefile's flags plus
``-Rpass-analysis=kernel-resource-usage`` and keep the compiler's stderr:

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off \
        -Rpass-analysis=kernel-resource-usage -c kernels.hip -o /tmp/k.o 2> head.log

    python tools/resource_usage.py parent.log head.log > profiles/<topic>/resource_usage.txt

The report lists every kernel of the second log that the first lacks (the new instantiations) with
its registers, scratch, occupancy and LDS, and every kernel both logs hold whose figures differ (none,
when a change leaves the existing instantiations alone). Exit status 1 if an old kernel changed or a
new one uses scratch. No GPU is needed.
"""
import re
import subprocess
import sys

FIELDS = ["TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]",
          "LDS Size [bytes/block]"]


def parse(path):
    out, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark: (?:\s*)Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z][^:]*): (\d+)", line)
        if m and cur is not None and m.group(1).strip() in FIELDS:
            cur[m.group(1).strip()] = int(m.group(2))
    return out


def demangle(names):
    if not names:
        return {}
    for tool in ("/opt/rocm/llvm/bin/llvm-cxxfilt", "c++filt"):
        try:
            r = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True)
            return dict(zip(names, r.stdout.splitlines()))
        except (OSError, subprocess.CalledProcessError):
            continue
    return {n: n for n in names}


def short(name):
    """The kernel's name and template arguments. The block-row kernels' trailing value-type argument
    ``double`` is the default of a parameter added after the integers (VT): such an instantiation is the
    kernel an older build names without it."""
    s = re.sub(r"^(void )?pamg::\(anonymous namespace\)::", "", name).split("(")[0]
    return re.sub(r"^(k_rows_bsr(?:_mc|_r)?<.*), double>$", r"\1>", s)


def by_template(log):
    """Keyed by the kernel's name and template arguments: a change may add trailing parameters to a
    kernel (another mangled name) without touching what an existing instantiation compiles to."""
    names = demangle(sorted(log))
    out = {}
    for k, v in log.items():
        assert short(names[k]) not in out, names[k]
        out[short(names[k])] = v
    return out


def main():
    old, new = by_template(parse(sys.argv[1])), by_template(parse(sys.argv[2]))
    names = {k: k for k in set(old) | set(new)}
    bad = 0
    print(f"kernels: {len(old)} before, {len(new)} after; {len(set(old) - set(new))} removed")
    changed = [k for k in sorted(old) if k in new and old[k] != new[k]]
    print(f"existing kernels whose resource usage changed: {len(changed)}")
    for k in changed:
        bad = 1
        print(f"  {short(names[k])}: {old[k]} -> {new[k]}")
    for k in sorted(set(old) - set(new)):
        bad = 1
        print(f"  removed: {short(names[k])}")
    added = sorted(set(new) - set(old), key=lambda k: names[k])
    print(f"new kernels: {len(added)}")
    print("  " + " | ".join(["kernel"] + FIELDS))
    for k in added:
        r = new[k]
        if r.get("ScratchSize [bytes/lane]", 0) != 0:
            bad = 1
        print("  " + " | ".join([short(names[k])] + [str(r.get(f, "?")) for f in FIELDS]))
    return bad


if __name__ == "__main__":
    sys.exit(main())
