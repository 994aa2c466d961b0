"""Compare the gfx950 assembly of a HIP unit's device functions between two builds, function by function.

    hipcc <the Makefile's HIPFLAGS> [-DTD_CHAIN_SKEW] --cuda-device-only -S chain_kernels.hip -o before.s   (parent commit)
    ... the same on this commit -> after.s
    python tools/asm_identity.py LABEL before.s after.s

Per function: the .LBB<n>_ label prefixes normalised, ; comments and __hip_cuid_* lines dropped.  Prints one
line per function (identical / differs: lines only before, lines only after / new / gone) and a last line
with the counts; exit status 1 if any function of the parent differs or is gone and --same was asked."""
import difflib
import re
import subprocess
import sys


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), stdout=subprocess.PIPE, text=True, check=True).stdout
        return dict(zip(names, (re.sub(r"\(.*", "", x.replace("(anonymous namespace)::", "").replace("tdstar::", ""))
                                .replace("void ", "") for x in out.splitlines())))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def functions(path):
    """name -> normalised body lines, in file order"""
    out, name, body = {}, None, []
    types = set()
    for line in open(path):
        m = re.match(r"\s*\.type\s+(\S+),@function", line)
        if m:
            types.add(m.group(1))
            continue
        m = re.match(r"^([A-Za-z_$][\w$.]*):", line)
        if m and m.group(1) in types and name is None:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if re.match(r"\s*\.Lfunc_end\d+:", line):
            out[name] = body
            name = None
            continue
        line = line.split(";")[0].rstrip()
        if not line.strip() or "__hip_cuid_" in line:
            continue
        body.append(re.sub(r"\.LBB\d+_", ".LBB_", line))
    return out


def main():
    args = [a for a in sys.argv[1:] if a != "--same"]
    label, before, after = args
    a, b = functions(before), functions(after)
    names = demangle(list(dict.fromkeys(list(a) + list(b))))
    same = differ = 0
    for n in names:
        if n not in a:
            print("%s: new  %s" % (label, names[n]))
        elif n not in b:
            differ += 1
            print("%s: gone  %s" % (label, names[n]))
        elif a[n] == b[n]:
            same += 1
            print("%s: identical  %s" % (label, names[n]))
        else:
            differ += 1
            d = list(difflib.unified_diff(a[n], b[n], lineterm="", n=0))
            minus = sum(1 for x in d if x.startswith("-") and not x.startswith("---"))
            plus = sum(1 for x in d if x.startswith("+") and not x.startswith("+++"))
            print("%s: differs (%d lines only before, %d only after; %d -> %d lines)  %s" %
                  (label, minus, plus, len(a[n]), len(b[n]), names[n]))
    print("%s: %d functions identical, %d differ or gone, of %d before and %d after" % (label, same, differ, len(a), len(b)))
    return 1 if differ and "--same" in sys.argv else 0


if __name__ == "__main__":
    sys.exit(main())
