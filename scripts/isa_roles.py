"""Instructions of one loop of a kernel's ISA, by role (count the decompress
walker's instructions per bin by role).  Input: device assembly with line tables, e.g.

  hipcc --offload-arch=gfx950 -O3 -std=c++17 -g -fPIC --cuda-device-only -S \\
      avrecode_amd/csrc/avr_k_decompress.hip -o /tmp/dec_g.s
  python scripts/isa_roles.py /tmp/dec_g.s 'slices_parallel_kernelILi1ELb0ELb0E' --anchor LINE CALLER
  python scripts/isa_roles.py /tmp/dec_g.s 'slices_parallel_kernelILi1ELb0ELb0E' --loop 4887

(LINE: avr_walker.h's line of `int b = rdec(e);` in sig_map's decompress map_loop, CALLER: the line
of the map_loop(...<int, 0>) call below it; --csrc DIR when the listing is of another tree's sources.)

Each instruction carries the inlining chain of its .loc comment; its role is the first frame of the
chain that falls in a known range of avr_walker.h / avr_slice_lds.h / avr_engine.h (ROLES below).  --anchor LINE CALLER
lists the innermost loops holding an instruction inlined from LINE through CALLER; --loop HDR prints
that loop's blocks (not those of loops nested in it) with their roles and the per-role sums.  The
code generation only: which blocks a bin runs is read off the listing."""
import argparse
import collections
import os
import re
import sys

W, L, E = "avr_walker.h", "avr_slice_lds.h", "avr_engine.h"
CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "avrecode_amd", "csrc")
# The roles are found in the sources as they stand, not by line numbers kept here (which every edit
# of the headers would move): (file, function, role) gives each definition of the function, all its
# overloads, to the role; (marker, [(pattern, role)...]) classifies the statements of one region of
# avr_walker.h -- from the line that holds the marker to the end of its brace block -- by their text.
FUNCS = [
    (E, "est_update", "est_update"),
    (E, "rd_get", "decision"), (E, "rd_consume", "decision"), (E, "in_byte", "decision"), (E, "hi32", "decision"),
    (E, "vhi32", "decision"), (E, "wave_all", "decision"), (E, "opaque_u32", "decision"),
    (W, "p1", "decision"), (W, "rdec", "decision"), (W, "rdec_lane", "decision"), (W, "rdec_mc", "decision"),
    (W, "rdec_bypass", "decision"), (L, "readlane64", "decision"),
    (L, "est_load", "est_lookup"), (L, "est_probe4", "est_lookup"), (L, "est_store", "est_store"),
    (L, "publish", "op_emit"), (L, "flush", "op_emit"), (L, "push_v", "op_emit"), (L, "stage", "op_emit"),
    (L, "flush_stage", "op_emit"), (L, "push", "op_emit"), (L, "push_v_raw", "op_emit"), (L, "op_map", "op_emit"),
    (L, "op_level", "op_emit"), (W, "publish", "op_emit"), (W, "push", "op_emit"), (W, "push_v", "op_emit"),
    (W, "wlane", "est_store"), (L, "wave_sync", "sync"),
]
STATEMENTS = [(r"est_load\(", "est_lookup"), (r"rdec(_lane|_bypass)?\(", "decision"), (r"est_update\(", "est_update"),
              (r"wlane\(|est_store\(|sh->etab", "est_store"), (r"push\(|mk \|=|mk = 0", "op_emit"),
              (r"\b(sc|lc|zo|i0|i1)\b.*=|const int idx = ", "context"), (r".", "bookkeeping")]
# the decompress significance map's loops (the second map_loop of sig_map) and the level loop
REGIONS = [("const uint32_t sop = opaque_u32", "auto map_loop = [&](auto K) {"),
           ("if constexpr (MODE == MODE_DECOMPRESS && !FLD) {", None)]


def block_end(lines, i):
    """Index of the line that closes the brace block opened on line i."""
    depth, opened = 0, False
    for j in range(i, len(lines)):
        for ch in lines[j].split("//")[0]:
            if ch == "{":
                depth, opened = depth + 1, True
            elif ch == "}":
                depth -= 1
                if opened and depth == 0:
                    return j
    return len(lines) - 1


def build_roles(csrc):
    roles, src = [], {}
    for f in (W, L, E):
        src[f] = open(os.path.join(csrc, f)).read().split("\n")
    for f, name, r in FUNCS:
        pat = re.compile(r"^\s*(AVR_FI|__device__|template|static|inline)\b[^=]*\b" + name + r"\s*\(")
        for i, line in enumerate(src[f]):
            if pat.match(line) and not line.rstrip().endswith(");"):
                k = i
                while "{" not in src[f][k] and k < i + 4:
                    k += 1
                roles.append((f, i + 1, block_end(src[f], k) + 1, r))
    lines = src[W]
    for first, then in REGIONS:
        i = next(k for k, l in enumerate(lines) if first in l)
        if then:
            i = next(k for k in range(i, len(lines)) if then in lines[k])
        for k in range(i, block_end(lines, i) + 1):
            text = lines[k].split("//")[0].strip()
            if text in ("", "{", "}", "};"):
                continue
            roles.append((W, k + 1, k + 1, next(r for p, r in STATEMENTS if re.search(p, text))))
    return roles


ROLES = []


def role(chain):
    for f, l in chain:
        for rf, a, b, r in ROLES:
            if f == rf and a <= l <= b:
                return r
    return "control"   # branches, joins and moves the line table gives to no helper (line 0)


def parse(path, kernel):
    blocks, cur, chain, on = [], None, (), False
    for line in open(path):
        s = line.strip()
        if not on:
            on = s.startswith("_ZN") and ":" in s and kernel in s.split(":")[0]   # the kernel's label
            continue
        if s.startswith(".Lfunc_end"):
            break
        m = re.match(r"^(\.LBB\d+_\d+|; %bb\.\d+):(.*)$", s)
        if m:
            lab = m.group(1).replace("; ", "")
            cur = {"label": lab, "id": re.split(r"[_.]", lab)[-1], "hdr": None, "ins": []}
            blocks.append(cur)
            mm = re.search(r"Header=BB\d+_(\d+)", m.group(2))
            if mm:
                cur["hdr"] = mm.group(1)
            continue
        if s.startswith(";") and cur is not None and not cur["ins"]:
            if "Loop Header" in s:
                cur["hdr"] = cur["id"]
            elif "in Loop:" in s:
                mm = re.search(r"Header=BB\d+_(\d+)", s)
                if mm:
                    cur["hdr"] = mm.group(1)
            continue
        if s.startswith(".loc"):
            c = s.split(";", 1)[1] if ";" in s else ""
            chain = tuple((a.split("/")[-1], int(b)) for a, b in re.findall(r"csrc/([\w./]+):(\d+):\d+", c))
            continue
        if not s or s.startswith(".") or s.startswith(";") or cur is None:
            continue
        cur["ins"].append((s.split()[0], chain))
    return blocks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("asm")
    ap.add_argument("kernel")
    ap.add_argument("--anchor", type=int, nargs=2)
    ap.add_argument("--loop")
    ap.add_argument("--csrc", default=CSRC, help="the sources the listing was compiled from (default: this tree's)")
    a = ap.parse_args()
    ROLES.extend(build_roles(a.csrc))
    blocks = parse(a.asm, a.kernel)
    print(f"{len(blocks)} blocks, {sum(len(b['ins']) for b in blocks)} instructions", file=sys.stderr)
    if a.anchor:
        line, caller = a.anchor
        hits = collections.Counter()
        for b in blocks:
            for _, ch in b["ins"]:
                ls = [l for f, l in ch if f == W]
                if line in ls and caller in ls:
                    hits[b["hdr"]] += 1
                    break
        for h, n in hits.most_common():
            print(f"loop {h}: {n} blocks with the anchor")
    if a.loop:
        tot = collections.Counter()
        for b in blocks:
            if b["hdr"] != a.loop:
                continue
            c = collections.Counter(role(ch) for _, ch in b["ins"])
            tot.update(c)
            print(f"{b['label']:14s} {len(b['ins']):3d}  " + " ".join(mn for mn, _ in b["ins"]))
            print(" " * 20 + ", ".join(f"{k} {v}" for k, v in c.most_common()))
        print("loop total:", dict(tot.most_common()))


if __name__ == "__main__":
    main()
