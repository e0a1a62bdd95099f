"""Per-kernel comparison of two device assembly listings of one source (hipcc --cuda-device-only -S
with cf2sim.build._compile_flags(src)): which kernel instances are byte-identical (function text and
.amdhsa_* descriptor), and the resources of those that are not.  Comments and the blanks before
them are not compared: they carry the function's position in the listing.
--rename PATTERN REPL (repeatable) rewrites the mangled symbols of AFTER with re.sub before they are
matched, for an instance whose template gained a defaulted parameter: the symbol is part of its own
text and descriptor, so it is rewritten there too.
python tools/isa_diff.py BEFORE.s AFTER.s [--label TEXT] [--rename PATTERN REPL]..."""
import argparse
import re
import shutil
import subprocess

RES = (("vgpr", "next_free_vgpr"), ("agpr_off", "accum_offset"), ("sgpr", "next_free_sgpr"),
       ("lds", "group_segment_fixed_size"), ("scratch", "private_segment_fixed_size"))


def kernels(path, renames=()):
    """{symbol: (function text, descriptor text, resources)} of every .amdhsa_kernel of the listing."""
    src = open(path).read()
    for sym in sorted(set(re.findall(r"\.amdhsa_kernel\s+(\w+)", src)), key=len, reverse=True):
        new = sym
        for pat, repl in renames:
            new = re.sub(pat, repl, new)
        if new != sym:
            src = re.sub(rf"\b{re.escape(sym)}\b", new, src)
    lines = src.split("\n")
    start = {}
    for n, l in enumerate(lines):
        m = re.match(r"^(\w+):\s*(;.*)?$", l)
        if m:
            start.setdefault(m.group(1), n)
    out = {}
    n = 0
    while n < len(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\w+)", lines[n])
        if not m:
            n += 1
            continue
        sym = m.group(1)
        e = n
        while ".end_amdhsa_kernel" not in lines[e]:
            e += 1
        desc = lines[n:e + 1]
        b = start[sym]
        f = b
        while not lines[f].startswith(".Lfunc_end"):
            f += 1
        res = {}
        for key, field in RES:
            for d in desc:
                mm = re.match(rf"\s*\.amdhsa_{field}\s+(\d+)", d)
                if mm:
                    res[key] = int(mm.group(1))
        for l in lines[f:f + 60]:
            mm = re.match(r";\s*Occupancy:\s*(\d+)", l)
            if mm:
                res["waves"] = int(mm.group(1))
                break
        # block labels carry the function's position in the listing, which moves with the order
        # of instantiation: not a difference of the kernel
        text = re.sub(r"\.LBB\d+_", ".LBB_", "\n".join(lines[b:f]))
        # so do the comments ("; in Loop: Header=BB11_5") and their column
        text = re.sub(r"[ \t]*;.*$", "", text, flags=re.M)
        # the section a function is emitted into (.text, or a comdat group of its own for a template's
        # instance) is no instruction either
        text = re.sub(r"^\s*\.(text|section)\b.*$", "", text, flags=re.M)
        out[sym] = (text, "\n".join(desc), res)
        n = e + 1
    return out


def demangle(syms):
    filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if filt is None:
        return {s: s for s in syms}
    r = subprocess.run([filt], input="\n".join(syms), capture_output=True, text=True, check=True).stdout.split("\n")
    return {s: re.sub(r"^(void )?cf2::", "", d) for s, d in zip(syms, r)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("--label", default="")
    ap.add_argument("--rename", nargs=2, action="append", default=[], metavar=("PATTERN", "REPL"))
    a = ap.parse_args()
    A, B = kernels(a.before), kernels(a.after, a.rename)
    names = demangle(sorted(set(A) | set(B)))
    same = [s for s in A if s in B and A[s][:2] == B[s][:2]]
    diff = [s for s in A if s in B and A[s][:2] != B[s][:2]]
    print(f"== {a.label}: {len(A)} -> {len(B)} kernel instances, {len(same)} identical, {len(diff)} changed, "
          f"{len(set(A) - set(B))} removed, {len(set(B) - set(A))} added")
    fam = {}
    for s in same:
        k = names[s].split("<")[0].split("(")[0]
        fam[k] = fam.get(k, 0) + 1
    for k in sorted(fam):
        print(f"identical  {k} x{fam[k]}")
    for s in diff:
        ra, rb = A[s][2], B[s][2]
        cols = " ".join(f"{k} {ra.get(k)}->{rb.get(k)}" if ra.get(k) != rb.get(k) else f"{k} {ra.get(k)}"
                        for k in ("vgpr", "agpr_off", "sgpr", "lds", "scratch", "waves"))
        print(f"changed    {names[s].split('(')[0]}: {cols}")
    for s in sorted(set(A) ^ set(B)):
        print(("removed    " if s in A else "added      ") + names[s].split("(")[0])


if __name__ == "__main__":
    main()
