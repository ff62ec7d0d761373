#!/bin/bash
# Device assembly of yaik_amd/csrc/yk_encode2.hip, a revision against the working tree (no GPU, about 25 s):
#   tools/same_isa.sh <rev> [extra compiler flags, e.g. -DYK_TEST_HOOKS]
# Both sources are compiled with the FLAGS of yaik_amd/csrc/Makefile; <rev>'s comes out of `git show` into a temporary tree together with the
# headers it includes.  The __hip_cuid_<hash> lines (the only thing two compiles of one source differ in) are dropped, and so is what moves when
# a kernel is added to the file without touching the others: the function's number in its labels, comments, a trailing template argument
# `false`.  Per kernel: identical / differs, then VGPRs, SGPRs, LDS bytes, scratch bytes, occupancy and code length of <rev> and of the working
# tree.  Exit status 1 when a kernel of <rev> differs or is gone.
set -o pipefail
REV=${1:?revision to compare the working tree against}; shift
ROOT=$(cd "$(dirname "$0")/.." && pwd)
CSRC=yaik_amd/csrc
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
FLAGS=$(sed -n 's/^FLAGS *:= *//p' "$ROOT/$CSRC/Makefile" | sed 's/\$(ARCH)/gfx950/')
T=$(mktemp -d); trap 'rm -rf "$T"' EXIT
mkdir -p "$T/$CSRC" "$T/include"
for f in $CSRC/yk_encode2.hip $CSRC/yk_common.h $CSRC/yk_udiv.h $CSRC/yk_curves.h $CSRC/yk_device.h include/yaik_hip.h include/yaik_hip_test.h; do
    git -C "$ROOT" show "$REV:$f" > "$T/$f" || exit 2
done
asm_of() { (cd "$1/$CSRC" && $HIPCC $FLAGS "${@:3}" --cuda-device-only -S yk_encode2.hip -o - | grep -v __hip_cuid > "$2"); }
asm_of "$T" "$T/old.s" "$@" & asm_of "$ROOT" "$T/new.s" "$@" & wait %1 && wait %2 || { echo "compile failed"; exit 2; }
python3 - "$T/old.s" "$T/new.s" "$REV" <<'PY'
import re, sys
def kernels(path):
    text = open(path).read()
    # a trailing template argument `false` that only one side has (WHOLE, round 8) is not a difference: <a, b, false> is compared as <a, b>
    text = re.sub(r"(yk_encode2_kernelILb[01]ELb[01])ELb0E", r"\1E", text)
    out = {}
    # a kernel's code: from its label to its .Lfunc_end; its figures: the .amdhsa_ descriptor and the comment block behind the code
    for m in re.finditer(r"^(_Z\w*yk_\w+):.*?^\.Lfunc_end\d+:\n", text, re.S | re.M):
        name, body = m.group(1), m.group(0)
        # labels carry the function's number in the file (.LBB<n>_<block>), which moves when a kernel is added in front of it: compared without
        # it, and without the comments that repeat it
        body = re.sub(r"Lfunc_end\d+", "Lfunc_end", re.sub(r"LBB\d+_", "LBBn_", re.sub(r"[ \t]*;.*$", "", body, flags=re.M)))
        tail = text[m.end():m.end() + 6000]
        def fig(pat, src=tail):
            g = re.search(pat, src)
            return int(g.group(1)) if g else None
        desc = re.search(r"\.amdhsa_kernel " + re.escape(name) + r"\n(.*?)\.end_amdhsa_kernel", text, re.S).group(1)
        out[name] = (body, {"VGPR": fig(r"; NumVgprs: (\d+)"), "SGPR": fig(r"; TotalNumSgprs: (\d+)"), "LDS": fig(r"\.amdhsa_group_segment_fixed_size (\d+)", desc),
                            "scratch": fig(r"; ScratchSize: (\d+)"), "occupancy": fig(r"; Occupancy: (\d+)"), "code": fig(r"; codeLenInByte = (\d+)")})
    return out
old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
bad = 0
for name in sorted(set(old) | set(new)):
    if name not in old or name not in new:
        print(f"{name}: only in {'the working tree' if name in new else sys.argv[3]}"); bad |= name not in new; continue   # a new kernel is no difference
    same = old[name][0] == new[name][0]
    bad |= not same
    print(f"{name}: {'identical' if same else 'differs'}")
    for tag, k in ((sys.argv[3], old), ("tree", new)):
        print(f"    {tag:12s}", " ".join(f"{a} {b}" for a, b in k[name][1].items()))
print("whole file (kernels, descriptors, metadata, data):", "identical" if open(sys.argv[1]).read() == open(sys.argv[2]).read() else "differs")
sys.exit(bad)
PY
