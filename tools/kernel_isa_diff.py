#!/usr/bin/env python3
"""Per-kernel ISA diff of the load kernels between two source trees (no GPU).

    tools/kernel_isa_diff.py <old>/native <new>/native

Compiles every loadgen/*.hip of both trees to gfx950 assembly with the
Makefile's HIPFLAGS, splits it per kernel symbol, strips comments,
.file/.ident lines and the per-build __hip_cuid_* symbol, and prints for each
kernel whether the text is identical, plus the register/scratch/LDS figures of
both sides. A plain text diff: it looks for no particular instruction. Exit
status is non-zero on any difference (text, metadata, or set of kernels).
"""
import difflib
import pathlib
import re
import subprocess
import sys

META = (".vgpr_count", ".agpr_count", ".sgpr_count",
        ".private_segment_fixed_size", ".group_segment_fixed_size")


def hipflags(native):
    mk = (native / "Makefile").read_text()
    var = lambda n: re.search(rf"^{n}\s*\?=\s*(.*)$", mk, re.M).group(1)
    return var("HIPFLAGS").replace("$(ARCH)", var("ARCH")).split()


def kernels(native):
    """{kernel: (stripped asm lines, {meta key: value})} over loadgen/*.hip."""
    out = {}
    for src in sorted((native / "loadgen").glob("*.hip")):
        asm = subprocess.run(
            ["hipcc", *hipflags(native), "--cuda-device-only", "-S", src.name,
             "-o", "-"], cwd=src.parent, check=True, stdout=subprocess.PIPE,
            text=True).stdout
        lines = []
        for ln in asm.splitlines():
            ln = ln.split(";", 1)[0].rstrip()
            if (ln and "__hip_cuid_" not in ln
                    and not re.match(r"\s*\.(file|ident)\b", ln)):
                lines.append(ln)
        meta = {}
        for entry in re.split(r"^  - (?=\.)", "\n".join(lines), flags=re.M)[1:]:
            name = re.search(r"^\s*\.name:\s*(\S+)", entry, re.M)
            if name:
                meta[name.group(1)] = {
                    k: m.group(1) if (m := re.search(
                        rf"^\s*{re.escape(k)}:\s*(\S+)", entry, re.M)) else "?"
                    for k in META}
        for name in meta:
            beg = lines.index(f"{name}:")
            end = lines.index("\t.end_amdhsa_kernel", beg)
            out[name] = (lines[beg:end + 1], meta[name])
    return out


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    old, new = (kernels(pathlib.Path(p)) for p in sys.argv[1:])
    bad = 0
    print("| kernel | text | " + " | ".join(k[1:] for k in META) + " |")
    print("|---|---|" + "---|" * len(META))
    for name in sorted(old.keys() | new.keys()):
        if name not in old or name not in new:
            print(f"| {name} | only in {'new' if name in new else 'old'} |")
            bad += 1
            continue
        (ta, ma), (tb, mb) = old[name], new[name]
        same = ta == tb
        bad += (not same) + (ma != mb)
        cells = [ma[k] if ma[k] == mb[k] else f"{ma[k]} -> {mb[k]}"
                 for k in META]
        print(f"| {name} | {'identical' if same else 'DIFFERENT'} "
              f"({len(ta)} / {len(tb)} lines) | " + " | ".join(cells) + " |")
        if not same:
            sys.stderr.write("".join(difflib.unified_diff(
                [x + "\n" for x in ta], [x + "\n" for x in tb],
                f"old/{name}", f"new/{name}", n=2)))
    print(f"\n{len(old)} / {len(new)} kernels, {bad} difference(s)")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
