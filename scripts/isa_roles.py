"""Instructions of one loop of a kernel's ISA, by role (count the decompress
walker's instructions per bin by role).  Input: device assembly with line tables, e.g.

  hipcc --offload-arch=gfx950 -O3 -std=c++17 -g -fPIC --cuda-device-only -S \\
      avrecode_amd/csrc/avr_k_decompress.hip -o /tmp/dec_g.s
  python scripts/isa_roles.py /tmp/dec_g.s 'slices_parallel_kernelILi1ELb0ELb0E' --anchor LINE CALLER
  python scripts/isa_roles.py /tmp/dec_g.s 'slices_parallel_kernelILi1ELb0ELb0E' --loop 4887
  python scripts/isa_roles.py /tmp/dec_g.s 'slices_parallel_kernelILi1ELb0ELb0E' --edges 4887
  python scripts/isa_roles.py /tmp/dec_g.s 'slices_parallel_kernelILi1ELb0ELb0E' --path 4887,4889,4893,4887
  python scripts/isa_roles.py /tmp/dec_g.s 'slices_parallel_kernelILi1ELb0ELb0E' --static

(LINE: avr_walker.h's line of `int b = rdec(e);` in sig_map's decompress map_loop, CALLER: the line
of the map_loop(...<int, 0>) call below it; --csrc DIR when the listing is of another tree's sources.
The compress kernel, 'slices_parallel_kernelILi0ELb0ELb0E' of avr_k_compress.hip, the same way: LINE
the `if (rdecide(sc)) {` of sig_map's first map_loop, or the `int b = rdecide(32 + i0);` of
residual_block's staged level loop with CALLER 0 -- any caller.)

Each instruction carries the inlining chain of its .loc comment; its role is the first frame of the
chain that falls in a known range of avr_walker.h / avr_slice_lds.h / avr_engine.h (ROLES below).  --anchor LINE CALLER
lists the innermost loops holding an instruction inlined from LINE through CALLER; --loop HDR prints
that loop's blocks (not those of loops nested in it) with their roles and the per-role sums.
--edges HDR prints the layout of that loop: its blocks in listing order, each with its branch
instructions, their targets, and the block it falls through to, so that the branches a path takes can
be told from those it merely passes; --path B1,B2,... walks a stated path (block numbers, in the order
a bin runs them) and counts its instructions, the branch instructions it executes and how many of
them are taken.  The code generation only: which blocks a bin runs is read off the listing
(DESIGN.md §4.3, §4.4)."""
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
    # the compress walker: the CABAC decoding engine is its decision, model ops its emission
    (E, "cd_decide", "decision"), (E, "cd_bypass", "decision"), (E, "cd_refill", "decision"), (E, "in_be32", "decision"),
    (E, "vtab_rec", "decision"), (E, "cabac_lps", "decision"), (E, "cabac_next", "decision"),
    (W, "rdecide", "decision"), (W, "crec", "decision"), (L, "op_model", "op_emit"),
]
STATEMENTS = [(r"est_load\(", "est_lookup"), (r"rdec(_lane|_bypass)?\(", "decision"), (r"est_update\(", "est_update"),
              (r"wlane\(|est_store\(|sh->etab", "est_store"), (r"rdecide\(|lbyp\(\)|cd_bypass\(", "decision"),
              (r"push\(|mk \|=|mk = 0|ring0\.|sigmask \|=", "op_emit"),
              (r"\b(sc|lc|zo|i0|i1)\b.*=|const int idx = ", "context"), (r".", "bookkeeping")]
# the decompress significance map's loops (the second map_loop of sig_map) and the level loop, then
# the compress side's: the first map_loop of sig_map and residual_block's staged level loop
REGIONS = [("const uint32_t sop = opaque_u32", "auto map_loop = [&](auto K) {"),
           ("if constexpr (MODE == MODE_DECOMPRESS && !FLD) {", None),
           ("uint64_t sigmask = 0;", "auto map_loop = [&](auto K) {"),
           ("} else if constexpr (MODE == MODE_COMPRESS && kStageLevels) {", None)]
# The per-block and per-macroblock code around those loops, for --static: helpers that
# belong to one role whole, and the statements of residual_block, nz_bits, sig_map's head, residual()
# and the macroblock loop of walk_slice by their text.  They come after the per-bin roles above, so
# a line of a per-bin region keeps its per-bin role.
BLOCK_FUNCS = [
    (W, "push_block", "blk:list_build"), (W, "list_luma", "blk:list_build"), (W, "blk_pos", "blk:list_build"),
    (W, "list_build", "blk:list_build"), (W, "edge_load", "mb:edge_load"),
    (W, "nnz_left", "blk:cbf_neighbours"), (W, "nnz_top", "blk:cbf_neighbours"), (W, "nnz_override", "blk:cbf_neighbours"),
    (W, "nb_cbp_left", "blk:cbf_neighbours"), (W, "nb_cbp_top", "blk:cbf_neighbours"),
    (W, "mnnz_left", "blk:nz_neighbours"), (W, "mnnz_top", "blk:nz_neighbours"), (W, "mnnz_prev", "blk:nz_neighbours"),
    (W, "rc_select", "blk:rc_select"), (W, "rc_writeback", "blk:rc_select"), (W, "rc_addr", "blk:rc_select"),
]
BLOCK_STATEMENTS = [
    (r"sh->blk\[|readlane\(blk2?_v|residual_block\(|\(b >> ", "blk:block_record"),
    (r"cur\.nnz\[|nz_v = wlane|cur\.mnnz\[n\]|mz_v = wlane|const uint32_t g = ", "blk:nnz_store"),
    (r"nz_v|nzn_v|nza|nzb|int bit = ", "blk:cbf_neighbours"),
    (r"mz_v|mzl_v|mzt_v|nb_left|nb_up|\b(li|ui|lv|av|has_left|has_above|pv)\b", "blk:nz_neighbours"),
    (r"T->(sig_base|last_base|abs_base|cbf_base|sig_est_base)", "blk:category_bases"),
    (r"c32\[lane\] = |w\.nz_v = 0|w\.mz_v = 0", "mb:clear"),
    (r"list_build\(|list_luma\(|push_block\(", "blk:list_build"),
    (r"edge_load\(", "mb:edge_load"),
    (r".", "blk:other"),
]
BLOCK_REGIONS = [("AVR_FI void residual_block(", None), ("AVR_FI int nz_bits(", None), ("AVR_FI int sig_map(", None),
                 ("AVR_FI void residual(int i16, int cbp) {", None)]
# (first line's marker, last line's marker, role) in walk_slice's macroblock loop
MB_REGIONS = [("// clear the current record (one dword per lane", "SPROF_ENDW(0, ps0);", "mb:clear"),
              ("// publish: bottom edge to the ring, full record to `left`", "PROF_ENDW(7, t7);", "mb:publish")]


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
    # the per-block and per-macroblock roles: after the per-bin ones (role() takes the first match)
    for f, name, r in BLOCK_FUNCS:
        pat = re.compile(r"^\s*AVR_FI\b[^=]*\b" + name + r"\s*\(")
        for i, line in enumerate(src[f]):
            if pat.match(line):
                roles.append((f, i + 1, block_end(src[f], i) + 1, r))
    for first, last, r in MB_REGIONS:
        i = next(k for k, l in enumerate(lines) if first in l)
        j = next(k for k in range(i, len(lines)) if last in lines[k])
        roles.append((W, i + 1, j + 1, r))
    for first, _ in BLOCK_REGIONS:
        i = next(k for k, l in enumerate(lines) if first in l)
        for k in range(i, block_end(lines, i) + 1):
            text = lines[k].split("//")[0].strip()
            if text in ("", "{", "}", "};"):
                continue
            roles.append((W, k + 1, k + 1, next(r for p, r in BLOCK_STATEMENTS if re.search(p, text))))
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
        cur["ins"].append((s.split()[0], chain, s.split(";")[0].strip()))
    return blocks


def branches(b):
    """(mnemonic, target block number) of the block's branch instructions, in order."""
    out = []
    for mn, _, text in b["ins"]:
        if mn.startswith("s_cbranch") or mn == "s_branch":
            m = re.search(r"\.LBB\d+_(\d+)", text)
            out.append((mn, m.group(1) if m else "?"))
    return out


def fall_through(blocks, i):
    """The block that follows in the listing, unless this one ends in an unconditional transfer."""
    last = blocks[i]["ins"][-1][0] if blocks[i]["ins"] else ""
    if last in ("s_branch", "s_endpgm", "s_setpc_b64") or i + 1 >= len(blocks):
        return None
    return blocks[i + 1]["id"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("asm")
    ap.add_argument("kernel")
    ap.add_argument("--anchor", type=int, nargs=2)
    ap.add_argument("--loop")
    ap.add_argument("--static", action="store_true", help="the whole kernel's instructions, LDS accesses and LDS waits by role")
    ap.add_argument("--edges", metavar="HDR", help="the loop's layout: each block's branches, targets and fall-through")
    ap.add_argument("--path", help="B1,B2,...: instructions, branch instructions and taken branches along these blocks")
    ap.add_argument("--csrc", default=CSRC, help="the sources the listing was compiled from (default: this tree's)")
    a = ap.parse_args()
    ROLES.extend(build_roles(a.csrc))
    blocks = parse(a.asm, a.kernel)
    print(f"{len(blocks)} blocks, {sum(len(b['ins']) for b in blocks)} instructions", file=sys.stderr)
    if a.static:
        # every instruction of the kernel once, by role: the per-block and per-macroblock code is
        # inlined at one site each, so its static count is what one block / macroblock can execute
        # at the most (all branches of the role together); LDS = ds_* instructions, waits = s_waitcnt
        # with an lgkmcnt operand
        tot, lds, waits = collections.Counter(), collections.Counter(), collections.Counter()
        for b in blocks:
            for mn, ch, text in b["ins"]:
                r = role(ch)
                tot[r] += 1
                lds[r] += mn.startswith("ds_")
                waits[r] += mn == "s_waitcnt" and "lgkmcnt" in text
        for r in sorted(tot, key=lambda r: (not r.startswith(("blk:", "mb:")), r)):
            print(f"{r:22s} {tot[r]:6d} instructions {lds[r]:4d} LDS {waits[r]:4d} lgkmcnt waits")
    if a.anchor:
        line, caller = a.anchor
        hits = collections.Counter()
        for b in blocks:
            for _, ch, _ in b["ins"]:
                ls = [l for f, l in ch if f == W]
                if line in ls and (caller in ls or not caller):
                    hits[b["hdr"]] += 1
                    break
        for h, n in hits.most_common():
            print(f"loop {h}: {n} blocks with the anchor")
    if a.loop:
        tot = collections.Counter()
        for b in blocks:
            if b["hdr"] != a.loop:
                continue
            c = collections.Counter(role(ch) for _, ch, _ in b["ins"])
            tot.update(c)
            print(f"{b['label']:14s} {len(b['ins']):3d}  " + " ".join(mn for mn, _, _ in b["ins"]))
            print(" " * 20 + ", ".join(f"{k} {v}" for k, v in c.most_common()))
        print("loop total:", dict(tot.most_common()))
    if a.edges:
        for i, b in enumerate(blocks):
            if b["hdr"] != a.edges:
                continue
            br, ft = branches(b), fall_through(blocks, i)
            roles = collections.Counter(role(ch) for _, ch, _ in b["ins"])
            print(f"{b['id']:>6s} {len(b['ins']):3d}  " + ("; ".join(f"{mn} -> {t}" for mn, t in br) or "-") +
                  f"  | falls through to {ft if ft else '(none)'}" + f"  | {roles.most_common(1)[0][0] if roles else ''}")
    if a.path:
        ids = a.path.split(",")
        at = {b["id"]: i for i, b in enumerate(blocks)}
        n_ins = n_br = n_taken = 0
        tot = collections.Counter()
        for k, x in enumerate(ids):
            b = blocks[at[x]]
            br, ft = branches(b), fall_through(blocks, at[x])
            nxt = ids[k + 1] if k + 1 < len(ids) else None
            if nxt is None and k and x == ids[0]:   # back at the loop's header: counted once
                break
            n_ins += len(b["ins"])
            tot.update(role(ch) for _, ch, _ in b["ins"])
            if nxt is None:
                break
            # the branches are executed in order until one is taken; the fall-through executes them all
            hit = next((j for j, (_, t) in enumerate(br) if t == nxt), None)
            if hit is None:
                if ft != nxt:
                    sys.exit(f"block {x} has no edge to {nxt} (branches {br}, falls through to {ft})")
                n_br += len(br)
                print(f"{x:>6s} -> {nxt:>6s}  falls through, past {len(br)} branch instruction(s)")
            else:
                n_br += hit + 1
                n_taken += 1
                print(f"{x:>6s} -> {nxt:>6s}  TAKEN {br[hit][0]}" + (f", past {hit} not taken" if hit else ""))
        print(f"path: {n_ins} instructions, {n_br} branch instructions executed, {n_taken} taken")
        print("path roles:", dict(tot.most_common()))


if __name__ == "__main__":
    main()
