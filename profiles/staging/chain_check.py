#!/usr/bin/env python3
"""Start-up of every kernel in a gfx950 assembly listing of hrt_kernels.hip
(hipcc -S --cuda-device-only with the flags of profiles/kres.sh):

  * loads issued before the first `s_waitcnt vmcnt` that is followed by a ds_write (the table's flight);
  * copy chains left: basic blocks that end in a backward branch and hold exactly one memory load, a
    `s_waitcnt vmcnt(0)` behind it and exactly one ds_write behind that.

usage: chain_check.py listing.s [kernel-name-substring ...]
"""
import re
import sys

LOAD = re.compile(r"^\s+(global_load|buffer_load|flat_load|scratch_load)_")
DSW = re.compile(r"^\s+ds_write")
VMW = re.compile(r"^\s+s_waitcnt\b.*vmcnt\((\d+)\)")
LABEL = re.compile(r"^(\.LBB\d+_\d+):")
BRANCH = re.compile(r"^\s+s_c?branch\w*\s+(\.LBB\d+_\d+)")


def kernels(path):
    name, body = None, []
    for line in open(path):
        m = re.match(r"^(_Z\w*hrt_\w+):", line)
        if m:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            yield name, body
            name = None
            continue
        body.append(line.rstrip("\n"))


def first_flight(body):
    """(loads before the first vmcnt wait that a ds_write follows, that wait's count, ds_writes before the barrier)"""
    loads = 0
    barrier = next((k for k, l in enumerate(body) if "s_barrier" in l), len(body))
    for n, line in enumerate(body):
        if LOAD.match(line):
            loads += 1
        m = re.match(r"^\s+s_cbranch_\w+\s+(\.LBB\d+_\d+)", line)
        if m:   # a block the compiler moved out of line (behind the barrier in the text): its loads are issued here
            at = next((k for k, l in enumerate(body) if l.startswith(m.group(1) + ":")), None)
            # (execnz: taken whenever a lane has work; the other kinds only where the block lies behind the barrier)
            if at is not None and at > n and ("execnz" in line or at > barrier):
                for later in body[at + 1:]:
                    if LABEL.match(later) or re.match(r"^\s+s_branch", later):
                        break
                    if LOAD.match(later):
                        loads += 1
        m = VMW.match(line)
        if m:
            for later in body[n + 1:]:
                if DSW.match(later):
                    return loads, int(m.group(1))
                if LOAD.match(later) or VMW.match(later) or LABEL.match(later) or "s_barrier" in later:
                    break
        if "s_barrier" in line:
            break
    return loads, None


def chains(body):
    blocks, cur, seen = [], None, set()
    for line in body:
        m = LABEL.match(line)
        if m:
            cur = [m.group(1)]
            blocks.append(cur)
            seen.add(m.group(1))
        elif cur is not None:
            cur.append(line)
    found = []
    for blk in blocks:
        ops = [l for l in blk[1:] if LOAD.match(l) or DSW.match(l) or VMW.match(l)]
        back = any((m := BRANCH.match(l)) and m.group(1) == blk[0] for l in blk[1:])
        if not back:
            continue
        kinds = ["L" if LOAD.match(l) else "D" if DSW.match(l) else ("W0" if VMW.match(l).group(1) == "0" else "W") for l in ops]
        if kinds.count("L") == 1 and kinds.count("D") == 1 and "W0" in kinds and kinds.index("L") < kinds.index("W0") < kinds.index("D"):
            found.append(blk[0])
    return found


def main():
    path, want = sys.argv[1], sys.argv[2:]
    total = 0
    for name, body in kernels(path):
        if want and not any(w in name for w in want):
            continue
        loads, cnt = first_flight(body)
        ch = chains(body)
        total += len(ch)
        print(f"{name[:64]:66s} loads in first flight {loads:3d}  wait vmcnt({cnt})  copy chains {len(ch)} {' '.join(ch)}")
    print("copy chains in all:", total)


if __name__ == "__main__":
    main()
