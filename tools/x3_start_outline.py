"""Outline of the start of a kernel from hipcc's assembly listing (-S --cuda-device-only): runs of loads, waits on vmcnt, runs of MFMAs with the
VALU instructions between them, labels and branches, from the kernel's entry up to its N-th MFMA -- enough to see in which order a ring is filled
ahead of a loop (profiles/x3_start.md).

usage: python tools/x3_start_outline.py LISTING.s SUBSTRING_OF_MANGLED_NAME [MFMAS=110] [ANCHOR=v_mfma_f32_32x32x16_bf16]
"""
import re
import sys


def outline(path, name, mfmas=110, anchor="v_mfma_f32_32x32x16_bf16"):
    lines = open(path).read().splitlines()
    starts = [i for i, l in enumerate(lines) if re.match(r"^_Z\w+:", l) and name in l]
    out = []
    for s in starts:
        sym = lines[s].split(":")[0]
        out.append(f"== {sym}")
        run, count, seen, valu = None, 0, 0, 0

        def flush():
            nonlocal run, count, valu
            if run:
                out.append(f"  {count:3d} x {run}" + (f"   (+ {valu} VALU between)" if valu else ""))
            run, count, valu = None, 0, 0

        # the product path: from the end of whatever path the listing puts ahead of it (the passengers' code) to the first MFMA of the kernel's product (anchor)
        end = next(i for i in range(s + 1, len(lines)) if lines[i].strip().startswith(".Lfunc_end"))
        first = next((i for i in range(s + 1, end) if lines[i].strip().startswith(anchor)), s + 1)
        begin = first
        while begin > s + 1 and not lines[begin].strip().startswith(("s_endpgm", "s_branch", "s_setpc")):
            begin -= 1
        for l in lines[begin + 1:end + 1]:
            t = l.strip()
            if t.startswith(".Lfunc_end"):
                break
            if t.startswith("s_endpgm"):
                flush(); out.append("        s_endpgm"); continue
            if re.match(r"^\.LBB\d+_\d+:", t):
                flush(); out.append(f"  {t.split(':')[0]}:"); continue
            if not t or t.startswith((";", ".")):
                continue
            op = t.split()[0]
            kind = None
            if op.startswith("global_load") or op.startswith("buffer_load"):
                kind = "load"
            elif op.startswith("v_mfma"):
                kind = "mfma"
            elif op.startswith("s_waitcnt") and "vmcnt" in t:
                flush(); out.append("        " + t.split(";")[0].strip()); continue
            elif op.startswith(("s_cbranch", "s_branch")):
                flush(); out.append("        " + t.split(";")[0].strip()); continue
            elif op.startswith(("s_memtime", "s_memrealtime")):
                flush(); out.append("        " + op); continue
            elif op.startswith("v_"):
                if run == "mfma":
                    valu += 1
                continue
            else:
                continue
            if kind != run:
                flush(); run = kind
            count += 1
            if kind == "mfma":
                seen += 1
                if seen >= mfmas:
                    break
        flush()
        kd = "\n".join(lines)
        m = re.search(r"\.amdhsa_kernel " + re.escape(sym) + r"\n(.*?)\.end_amdhsa_kernel", kd, re.S)
        if m:
            for k in ("next_free_vgpr", "accum_offset", "private_segment_fixed_size"):
                v = re.search(k + r" (\S+)", m.group(1))
                out.append(f"  {k} {v.group(1) if v else '?'}")
    return "\n".join(out)


if __name__ == "__main__":
    print(outline(sys.argv[1], sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 110, *sys.argv[4:5]))
