#!/usr/bin/env python3
"""Compare the kernels of two directories of gfx950 assembly (`make asmcheck` writes build/asm/*.hip.s).

    python3 tools/asm_diff.py OLD_DIR NEW_DIR [--rename OLD_SYMBOL=NEW_SYMBOL ...] [--show N]

Per kernel symbol: the descriptor's resources (VGPRs, SGPRs, accum offset, LDS, scratch) must be equal and the
instruction stream identical once comments, debug lines and basic-block label numbers are normalised away.
Prints one line per kernel that differs or exists on one side only (with --show N: the first N lines of the stream's
unified diff), a summary per file, and exits 1 if anything differs.
"""
import difflib
import pathlib
import re
import sys

RESOURCES = ("next_free_vgpr", "next_free_sgpr", "accum_offset", "group_segment_fixed_size", "private_segment_fixed_size")


def kernels(path):
    """symbol -> (resources, normalised instruction lines)"""
    text = path.read_text().splitlines()
    res, body = {}, {}
    cur, lines, desc = None, [], None
    for raw in text:
        line = raw.split(";", 1)[0].rstrip()
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            res[m.group(1)] = {}
            desc = m.group(1)
            continue
        m = re.match(r"\s*\.amdhsa_(\w+)\s+(\S+)", line)
        if m and desc is not None and m.group(1) in RESOURCES:
            res[desc][m.group(1)] = m.group(2)
            continue
        m = re.match(r"(\w+):$", line)
        if m and not line.startswith(".L") and cur is None:
            cur, lines = m.group(1), []
            continue
        if cur is None:
            continue
        if re.match(r"\.Lfunc_end\d+:", line):
            body[cur] = lines
            cur = None
            continue
        s = line.strip()
        if not s or re.match(r"\.(loc|file|cfi_\w+|p2align|section|text)\b", s) or re.match(r"\.Ltmp\d+:", s):
            continue
        lines.append(s)
    out = {}
    for sym, r in res.items():
        if not body.get(sym):
            sys.exit("%s: no instructions found for kernel %s" % (path, sym))
        labels = {}
        norm = [re.sub(r"\.LBB\d+_\d+", lambda m: labels.setdefault(m.group(0), "L%d" % len(labels)), l) for l in body[sym]]
        out[sym] = (r, norm)
    return out


def main(argv):
    show, renames, dirs = 0, {}, []
    it = iter(argv)
    for a in it:
        if a == "--rename":
            old, new = next(it).split("=")
            renames[old] = new
        elif a == "--show":
            show = int(next(it))
        else:
            dirs.append(pathlib.Path(a))
    if len(dirs) != 2:
        sys.exit(__doc__)
    bad = 0
    for old_file in sorted(dirs[0].glob("*.s")):
        new_file = dirs[1] / old_file.name
        if not new_file.exists():
            print("%s: missing in %s" % (old_file.name, dirs[1]))
            bad += 1
            continue
        old = {renames.get(k, k): v for k, v in kernels(old_file).items()}
        new = kernels(new_file)
        same = 0
        for sym in sorted(set(old) | set(new)):
            if sym not in old or sym not in new:
                print("%s: %s only in %s" % (old_file.name, sym, dirs[1] if sym in new else dirs[0]))
                bad += 1
                continue
            (r0, b0), (r1, b1) = old[sym], new[sym]
            if r0 == r1 and b0 == b1:
                same += 1
                continue
            bad += 1
            print("%s: %s DIFFERS: resources %s; instructions %d -> %d" %
                  (old_file.name, sym, "equal" if r0 == r1 else "%s -> %s" % (r0, r1), len(b0), len(b1)))
            for l in list(difflib.unified_diff(b0, b1, lineterm="", n=1))[2:2 + show]:
                print("    " + l)
        print("%s: %d kernels identical, %d in all" % (old_file.name, same, len(set(old) | set(new))))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
