#!/usr/bin/env python3
"""Register / spill / scratch / LDS figures of every kernel in a built libmuavta.so, read from the code object's metadata
(builder's tool; no recompile).  usage: kernel_meta.py [path/to/libmuavta.so] [substring ...]
       kernel_meta.py NEW.so --diff OLD.so    both tables row by row, then every function's instruction stream (see diff())
       kernel_meta.py NEW.so --diff OLD.so --by-name   the same with the functions matched by name: for a build that ADDS instantiations"""
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"


# The template arguments behind the tile — k_rollout<TL, REC, AL>, k_allocate<TL, AL>, k_pair_scores<TL, POL> — printed as the tags the
# committed tables use: REC = the recording rollout, BL = AllocBaseline, PM = AllocLearned<POL>, and with it (or for k_pair_scores alone)
# CX = PolContextPair, CO = PolCoalition, W = the variant over the wide 48 x 64 token pads (PolPairWide, PolContextPairWide), UW =
# AllocUrgencyWide (Urgency-Pair at those pads).  AllocHungarian and PolPair print nothing.
TAGS = (("REC", "Lb1E"), ("BL", "AllocBaseline"), ("UW", "AllocUrgencyWide"), ("PM", "AllocLearned"), ("RL", "AllocLearnedRl"), ("CX", "PolContextPair"), ("CO", "PolCoalition"),
        ("W", "PairWide"))  # RL = AllocLearnedRl<POL>: the rollout that records the RL transitions (printed behind PM)


def short(name):
    m = re.search(r"(k_\w+?)I4TileILi(\d+)ELi(\d+)E(?:L[ib]\d+E)*E(.*?)Ev", name)
    if m:
        tags = "".join(f",{t}" for t, s in TAGS if s in m.group(4))
        bits = re.findall(r"Lb(\d)E", m.group(4))
        if len(bits) > 1 and re.fullmatch(r"(Lb\dE)+E*", m.group(4)):  # a build from before the tag types: one bool each, in this order (--diff against such a build)
            tags = "".join(f",{t}" for t, b in zip(("REC", "BL", "PM", "CX", "CO")[-len(bits):], bits) if b == "1")
        return f"{m.group(1)}<{m.group(2)}x{m.group(3)}{tags}>"
    m = re.search(r"N_1\d+(k_\w+?)E", name)
    return m.group(1) if m else name[:60]


def code_object(so, d):
    fat, co = os.path.join(d, "fat.bin"), os.path.join(d, "k.co")
    subprocess.check_call(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", so, fat])
    subprocess.check_call([f"{LLVM}/clang-offload-bundler", "--type=o", f"--input={fat}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}", "--unbundle"])
    return co


def table(so, subs=()):
    with tempfile.TemporaryDirectory() as d:
        notes = subprocess.check_output([f"{LLVM}/llvm-readelf", "--notes", code_object(so, d)], text=True)
    rows = [f"{'kernel':34s} {'VGPR':>5s} {'vspill':>6s} {'SGPR':>5s} {'sspill':>6s} {'scratch B':>9s} {'LDS B':>7s}"]
    for blk in notes.split("  - .agpr_count:")[1:]:
        def f(key):
            m = re.search(rf"\.{key}:\s+(\S+)", blk)
            return m.group(1) if m else "?"
        name = short(f("name"))
        if subs and not any(s in name for s in subs):
            continue
        rows.append(f"{name:34s} {f('vgpr_count'):>5s} {f('vgpr_spill_count'):>6s} {f('sgpr_count'):>5s} {f('sgpr_spill_count'):>6s} {f('private_segment_fixed_size'):>9s} {f('group_segment_fixed_size'):>7s}")
    return rows


def streams(so):
    """[(symbol, [instruction text])] of every function in the code object, in order.  Masked: the 32-bit literal of an s_add_u32 / s_addc_u32
    within three instructions after an s_getpc_b64 (a pc-relative address: it moves with .rodata and with the functions in front)."""
    with tempfile.TemporaryDirectory() as d:
        dis = subprocess.check_output([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", code_object(so, d)], text=True)
    funcs = []
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]* ?<(.+)>:$", line)
        if m:
            funcs.append((m.group(1), []))
        elif funcs and line.startswith("\t"):
            funcs[-1][1].append(re.sub(r"\s*//.*$", "", line).strip())
    for _, body in funcs:
        for i, ins in enumerate(body):
            if ins.startswith("s_getpc_b64"):
                for j in range(i + 1, min(i + 4, len(body))):
                    if re.match(r"s_addc?_u32 ", body[j]):
                        body[j] = body[j].rsplit(",", 1)[0] + ", <pcrel>"
    return funcs


def diff(new, old):
    """Same machine code?  (a) the two tables agree row for row; (b) every function's instruction stream is identical — per function, in
    order, symbol names ignored, nothing masked but the pc-relative literals (streams()).  Exit status 1 if either differs."""
    ta, tb = table(new), table(old)
    print(f"new: {new}\nold: {old}\n\n(a) kernel table: {len(ta) - 1} kernels new, {len(tb) - 1} old")
    bad = len(ta) != len(tb)
    for a, b in zip(ta, tb):
        same = a == b
        bad |= not same
        print(a if same else f"{a}   <-- old: {b}")
    fa, fb = streams(new), streams(old)
    n_ins = sum(len(body) for _, body in fa)
    print(f"\n(b) instruction streams: {len(fa)} functions new, {len(fb)} old; {n_ins} instructions new")
    differ = 0
    for (na, ia), (nb, ib) in zip(fa, fb):
        if ia != ib:
            differ += 1
            first = next((k for k, (x, y) in enumerate(zip(ia, ib)) if x != y), min(len(ia), len(ib)))
            print(f"DIFFERENT {short(na)} / {short(nb)}: {len(ia)} against {len(ib)} instructions, {sum(x != y for x, y in zip(ia, ib))} differ in place, first at {first}")
    bad |= differ != 0 or len(fa) != len(fb)
    print(f"{len(fa) - differ} of {len(fa)} functions identical instruction for instruction" + ("" if differ else " (all)"))
    return 1 if bad else 0


def diff_by_name(new, old):
    """diff() for a build that adds kernels: every kernel of `old` must be in `new` under the same name with the same table row and the
    same instruction stream (the k-th function of a name against the k-th of that name); what only `new` has is listed with its row.
    Exit status 1 if a kernel of `old` is missing or differs in its row; differing streams are listed and counted, not fatal here: the
    caller decides which kernels may change."""
    ta, tb = table(new), table(old)
    rows_b = {r.split()[0]: r for r in tb[1:]}
    names_a = [r.split()[0] for r in ta[1:]]
    print(f"new: {new}\nold: {old}\n\n(a) kernel table: {len(ta) - 1} kernels new, {len(tb) - 1} old")
    print(ta[0])
    bad = 0
    for r in ta[1:]:
        b = rows_b.get(r.split()[0])
        print(r + ("   <-- NEW" if b is None else "" if b == r else f"   <-- old: {b}"))
        bad |= b is not None and b != r
    for n in rows_b:
        if n not in names_a:
            print(f"MISSING {n}")
            bad = 1

    def grouped(funcs):
        g = {}
        for sym, body in funcs:
            g.setdefault(short(sym), []).append(body)
        return g
    ga, gb = grouped(streams(new)), grouped(streams(old))
    same = differ = 0
    print(f"\n(b) instruction streams by name: {sum(map(len, ga.values()))} functions new, {sum(map(len, gb.values()))} old")
    for n, bodies in gb.items():
        for k, ib in enumerate(bodies):
            ia = ga.get(n, [])[k] if k < len(ga.get(n, [])) else None
            if ia == ib:
                same += 1
                continue
            differ += 1
            if ia is None:
                print(f"MISSING {n}")
                bad = 1
            else:
                first = next((i for i, (x, y) in enumerate(zip(ia, ib)) if x != y), min(len(ia), len(ib)))
                print(f"DIFFERENT {n}: {len(ia)} against {len(ib)} instructions, {sum(x != y for x, y in zip(ia, ib))} differ in place, first at {first}")
    print(f"{same} of {same + differ} functions of the old build identical instruction for instruction in the new one" + ("" if differ else " (all)"))
    return bad


def main():
    args = sys.argv[1:]
    if "--diff" in args:
        i = args.index("--diff")
        sys.exit((diff_by_name if "--by-name" in args else diff)(args[0], args[i + 1]))
    so = args[0] if args and args[0].endswith(".so") else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "multi-uav-ta-gym-env_amd", "libmuavta.so")
    print("\n".join(table(so, [a for a in args if not a.endswith(".so")])))


if __name__ == "__main__":
    main()
