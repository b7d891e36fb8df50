"""Per-kernel comparison of two builds' device assembly.

    python tools/isa_diff.py OLD_ASM_DIR NEW_ASM_DIR

Reads the *-hip-amdgcn-amd-amdhsa-gfx950.s listings that build_hip() leaves in
build/asm (one per .hip file), splits them at the function symbols and prints
one line per listing and mangled name: `same` or `DIFF (n lines)`, then both
builds' VGPRs / SGPRs / scratch bytes / LDS bytes / occupancy (old -> new where
they differ).  Before comparing, everything from `;` to the end of a line and
trailing blanks go, and the .LBB labels are renumbered by first appearance
within the function.  Exit status 1 when a function differs or exists on one
side only.  It compares text; it knows nothing about instructions."""
import difflib
import glob
import os
import re
import sys

SUFFIX = "-hip-amdgcn-amd-amdhsa-gfx950.s"
RESOURCES = (".amdhsa_next_free_vgpr", ".amdhsa_next_free_sgpr", ".amdhsa_private_segment_fixed_size",
             ".amdhsa_group_segment_fixed_size", "; Occupancy:")


def functions(text):
    """{symbol: (normalised body lines, resource figures)} of one listing"""
    lines = text.splitlines()
    code_of = [line.split(";")[0].rstrip() for line in lines]
    starts = []  # (line of `symbol:`, symbol)
    for i, code in enumerate(code_of):
        m = re.match(r"\s*\.type\s+([\w.$]+),@function$", code)
        if m:
            starts.append((code_of.index(m.group(1) + ":", i), m.group(1)))
    out = {}
    for k, (begin, name) in enumerate(starts):
        end = starts[k + 1][0] if k + 1 < len(starts) else len(lines)
        body, res, labels, in_body = [], {}, {}, True
        for line, code in zip(lines[begin:end], code_of[begin:end]):
            for key in RESOURCES:
                if line.strip().startswith(key):
                    res[key] = line.strip()[len(key):].strip()
            if line.startswith(".Lfunc_end"):
                in_body = False  # (what follows restates the resources as .set lines and comments)
            if in_body and code:
                body.append(re.sub(r"\.LBB\d+_\d+", lambda m: labels.setdefault(m.group(0), f".L{len(labels)}"), code))
        out[name] = (body, [res.get(key, "-") for key in RESOURCES])
    return out


def listing(directory):
    out = {}
    for path in sorted(glob.glob(os.path.join(directory, "*" + SUFFIX))):
        unit = os.path.basename(path)[:-len(SUFFIX)]
        with open(path) as f:
            for name, v in functions(f.read()).items():
                out[(unit, name)] = v
    return out


def main(old_dir, new_dir):
    old, new = listing(old_dir), listing(new_dir)
    bad = 0
    print("unit symbol verdict | vgpr sgpr scratch lds occupancy")
    for key in sorted(set(old) | set(new)):
        if key not in old or key not in new:
            verdict, res = "ONLY IN " + ("old" if key in old else "new"), (old.get(key) or new[key])[1]
            bad += 1
        else:
            (a, ra), (b, rb) = old[key], new[key]
            n = sum(1 for d in difflib.unified_diff(a, b, lineterm="", n=0)
                    if d[:1] in "+-" and d[:3] not in ("+++", "---"))
            verdict = "same" if a == b else f"DIFF ({n} lines)"
            bad += a != b
            res = [x if x == y else f"{x}->{y}" for x, y in zip(ra, rb)]
        print(key[0], key[1], verdict, "|", " ".join(res))
    print(f"{len(set(old) | set(new))} functions, {bad} differ or are missing")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
