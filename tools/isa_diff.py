"""Per-kernel comparison of two builds' gfx950 assembly (no GPU needed): registers, spills, scratch, LDS, instruction counts, the size
of every loop that issues MFMAs, and whether the instruction streams are identical once symbol names are normalised.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -x hip -S --cuda-device-only [-fno-honor-nans] -o old/attention.s <old tree>/csrc/attention.hip
    ... the same for the new tree ...
    python tools/isa_diff.py old/attention.s new/attention.s [--drop-arg attn_fused_kernel:4]

--drop-arg NAME:I removes template argument I (0-based, integer arguments only) from the OLD side's mangled names of kernel NAME, for a
refactor that retires a template parameter.  Exit status 1 when a kernel is missing on one side or any figure of the new side is larger."""
import re
import sys

FIELDS = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")


def kernels(path):
    text = open(path).read()
    meta = text[text.index("amdhsa.kernels:"):]
    lines = text.split("\n")
    start = {m.group(1): i for i, l in enumerate(lines) if (m := re.match(r"(_Z\w+|[A-Za-z]\w*):", l))}
    out = {}
    for blk in re.split(r"\n  - ", meta)[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        if not name:
            continue
        name = name.group(1)
        info = {k: int(m.group(1)) if (m := re.search(rf"\.{k}:\s+(\d+)", blk)) else 0 for k in FIELDS}
        i0 = start[name]
        i1 = next(i for i in range(i0, len(lines)) if lines[i].startswith(".Lfunc_end"))
        body = []
        for l in lines[i0 + 1:i1]:
            l = re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"_Z\w+", "SYM", l.split(";")[0])).rstrip()
            if l.strip() and not re.match(r"\s+\.", l):        # labels and instructions, no directives
                body.append(l)
        info["stream"] = body
        info["instructions"] = sum(1 for l in body if l.startswith("\t"))
        labels = {m.group(1): i for i, l in enumerate(body) if (m := re.match(r"(\.LBB_\d+):", l))}
        loops = []
        for i, l in enumerate(body):
            m = re.search(r"s_c?branch\w* (\.LBB_\d+)", l)
            if m and labels.get(m.group(1), i) < i:
                loop = body[labels[m.group(1)]:i + 1]
                if any("v_mfma" in x for x in loop):
                    loops.append((sum("v_mfma" in x for x in loop), sum(1 for x in loop if x.startswith("\t"))))
        info["mfma_loops"] = loops
        out[name] = info
    return out


def main(argv):
    drop = [a.split(":") for i, a in enumerate(argv) if argv[i - 1] == "--drop-arg"]
    old, new = kernels(argv[1]), kernels(argv[2])
    for kname, idx in drop:
        for n in [n for n in old if kname in n]:
            args = re.match(rf"(.*{kname}I)((?:L[ib]\d+E)+)(E.*)", n)
            if not args:
                continue
            parts = re.findall(r"L[ib]\d+E", args.group(2))
            del parts[int(idx)]
            old[args.group(1) + "".join(parts) + args.group(3)] = old.pop(n)
    bad = 0
    print(f"{argv[1]} -> {argv[2]}: {len(old)} -> {len(new)} kernels")
    for n in sorted(set(old) | set(new)):
        if n not in old or n not in new:
            print(f"{n}: only in {'old' if n in old else 'new'}")
            bad = 1
            continue
        o, h = old[n], new[n]
        same = o["stream"] == h["stream"]
        worse = [k for k in FIELDS + ("instructions",) if h[k] > o[k]]
        if len(h["mfma_loops"]) == len(o["mfma_loops"]):
            worse += [f"mfma loop {i}" for i, (a, b) in enumerate(zip(o["mfma_loops"], h["mfma_loops"])) if b[1] > a[1]]
        elif not same:
            worse.append("mfma loops differ in number: compare by hand")
        bad |= bool(worse)
        fig = lambda d: (f"vgpr {d['vgpr_count']} agpr {d['agpr_count']} sgpr {d['sgpr_count']} spill v{d['vgpr_spill_count']}/s{d['sgpr_spill_count']} "
                         f"scratch {d['private_segment_fixed_size']} lds {d['group_segment_fixed_size']} instr {d['instructions']} "
                         f"mfma-loops(mfma,instr) {d['mfma_loops']}")
        print(n)
        print(f"    {'identical stream; ' + fig(h) if same else 'old: ' + fig(o)}")
        if not same:
            print(f"    new: {fig(h)}{'   WORSE: ' + ', '.join(worse) if worse else ''}")
    return bad


if __name__ == "__main__":
    sys.exit(main(sys.argv))
