"""Compare two logs of `hipcc -Rpass-analysis=kernel-resource-usage -c yaik_amd/csrc/yk_decode.hip` (parent, this tree): every kernel of the parent
must be there with the same figures, and no kernel may use scratch.  Prints a table (names through `c++filt -p`); exit status 1 on a difference.
profiles/decode_prepared/resource_usage.txt is its header plus this script's output.
usage: resource_diff.py <parent.log> <new.log>"""
import re
import subprocess
import sys


def parse(path):
    out, name = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark:\s+(?:Function Name: (\S+)|([^:]+): (\S+)) \[-Rpass", line)
        if not m:
            continue
        if m.group(1):
            name = m.group(1)
            out[name] = {}
        elif name:
            out[name][m.group(2).strip()] = m.group(3)
    return out


def demangled(names):
    """mangled name -> readable name without the parameter list; the mangled name where c++filt is missing"""
    names = sorted(names)
    try:
        got = subprocess.run(["c++filt", "-p"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    except (OSError, subprocess.CalledProcessError):
        got = names
    return dict(zip(names, got))


def figures(v):
    g = v.get
    return (f"SGPRs {g('TotalSGPRs')} VGPRs {g('VGPRs')} AGPRs {g('AGPRs')} scratch {g('ScratchSize [bytes/lane]')} occupancy {g('Occupancy [waves/SIMD]')} "
            f"spills {g('SGPRs Spill')}/{g('VGPRs Spill')} LDS {g('LDS Size [bytes/block]')}")


def main():
    old, new = parse(sys.argv[1]), parse(sys.argv[2])
    name = demangled(set(old) | set(new))
    bad = 0
    for k in sorted(name, key=lambda k: (name[k], k)):
        if k not in new:
            print(f"MISSING   {name[k]}"); bad += 1
        elif k not in old:
            print(f"new       {name[k]}  {figures(new[k])}")
        elif old[k] != new[k]:
            print(f"DIFFERENT {name[k]}\n   parent {figures(old[k])}\n   new    {figures(new[k])}"); bad += 1
        else:
            print(f"same      {name[k]}  {figures(new[k])}")
    scratch = [name[k] for k, v in new.items() if v.get("ScratchSize [bytes/lane]", "0") != "0"]
    print(f"{len(old)} kernels in the parent, {len(new)} now, {bad} changed or missing, kernels with scratch: {scratch or 'none'}")
    return 1 if bad or scratch else 0


if __name__ == "__main__":
    sys.exit(main())
