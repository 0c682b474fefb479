"""Helpers of tests/test_uutigs_frags.py: the fragment build of mhmkc_uutigs_frags (include/mhmkc.h)
restated in Python over the oracle's table of all reads and the reference's owner of every row.

frags_ref restates stages 1 and 2 (the claims, the local ranking): per rank the open and closed fragments, the local
cycles and the cross links, and per contig its fragments in order with strand and offset. layout_ref lays the fragments
out by stages 4 to 6 (the fragment graph, the cycle rotation, the row map, the bases); its result is compared with
uutigs_ref, the single-rank rule over the same table, so the decomposition is tested without a GPU.
"""
from __future__ import annotations

import functools

import numpy as np

import mhm2_proxy_amd as m
import oracle_lib as O
from common import oracle_table
from mr_uutig_worker import case_reads as worker_case_reads
from query_lib import NO_ROW, OK, RC, links_ref
from uutig_lib import circular_set, pack_reads, revcomp, uutigs_ref

EXTRA_CASES = [("circ23", 21), ("tandem", 21)]


@functools.lru_cache(maxsize=None)
def case_reads(setname: str, k: int):
    """The cases of test_uutigs_ranks.py and the two this build adds: a cycle of 23 rows, and a tandem repeat whose five
    rows form a cycle on one rank."""
    if setname == "circ23":
        return circular_set(23, seed=3)
    if setname == "tandem":
        return pack_reads(["ACGGT" * 30] * 3)
    return worker_case_reads(setname, k)


@functools.lru_cache(maxsize=None)
def cpu_case(setname: str, k: int):
    """The oracle's table of all reads of a case, its links and the restated uutigs (computed once, never changed)."""
    b, o = case_reads(setname, k)
    t = oracle_table(b, o, k)
    nxt, status, _ = links_ref(t)
    return t, nxt, status, uutigs_ref(t, nxt, status)


def table_ranks(t, world: int) -> np.ndarray:
    if not len(t):
        return np.zeros(0, dtype=np.int64)
    return np.asarray(O.target_ranks(np.ascontiguousarray(t.keys[:, :t.k // 32 + 1]), t.k, world)).astype(np.int64)


def frags_ref(t: m.KmerTable, nxt: np.ndarray, status: np.ndarray, owner: np.ndarray, world: int = 0) -> dict:
    """Stages 1 and 2 over the union table: rows are the union's, owner[row] the rank that holds it (of `world` ranks)."""
    n, k = len(t), t.k
    strs = m.keys_to_strings(t.keys, k) if n else []
    counts = [int(x) for x in t.counts]
    owner = [int(x) for x in owner]
    world = max(world, max(owner) + 1 if owner else 1)
    walkable = [chr(int(t.left[i])) in "ACGT" and chr(int(t.right[i])) in "ACGT" for i in range(n)]

    def entry(i, d):  # the port an OK port enters
        st = int(status[d, i])
        if (st & ~RC) != OK:
            return None
        return int(nxt[d, i]), d ^ (1 if st & RC else 0) ^ 1

    # stage 1: the claims every rank receives, and the ports they cross-link
    claims = set()
    for i in range(n):
        for d in (0, 1):
            en = entry(i, d)
            if en is not None and owner[en[0]] != owner[i]:
                claims.add((owner[en[0]], owner[i], i, d, en[0], en[1]))  # (to, from, row, d, entered row, e)
    cross = {}
    for j in range(n):
        for e in (0, 1):
            en = entry(j, e)
            if en is not None and owner[en[0]] != owner[j] and (owner[j], owner[en[0]], en[0], en[1], j, e) in claims:
                cross[(j, e)] = en
    # stage 2: the local links (a neighbour on another rank is an end) and their mutual-link rule
    link = {}
    for i in range(n):
        for d in (0, 1):
            en = entry(i, d)
            if en is None or owner[en[0]] != owner[i] or en == (i, d):
                continue
            back = entry(*en)
            if back == (i, d) and owner[en[0]] == owner[i]:
                link[(i, d)] = en

    def travel(i, d):  # the rows met leaving (i, d), each with the port travel leaves it through
        out = [(i, d)]
        while (i, d) in link:
            j, e = link[(i, d)]
            i, d = j, e ^ 1
            if (i, d) == out[0]:
                return out, True
            out.append((i, d))
        return out, False

    seen = [False] * n
    frags = []  # per fragment: rank, start, placed rows (lp, row, lrc), cyc, ends, peers
    for i in range(n):
        if not walkable[i] or seen[i]:
            continue
        left, cyc = travel(i, 0)
        rows = [r for r, _ in left]
        if not cyc:
            right, _ = travel(i, 1)
            rows += [r for r, _ in right[1:]]
        s = min(rows, key=lambda r: strs[r])
        chain, cyc = travel(s, 0)  # leftwards from the start (all the way round on a cycle)
        mrows = len(rows)
        placed = [(len(chain) - 1 - x, r, 0 if d == 0 else 1) for x, (r, d) in enumerate(chain)]
        if not cyc:
            rchain, _ = travel(s, 1)
            placed += [(len(chain) - 1 + x, r, 0 if d == 1 else 1) for x, (r, d) in enumerate(rchain) if x]
        placed.sort()
        assert len(placed) == mrows and [p for p, _, _ in placed] == list(range(mrows))
        for _, r, _ in placed:
            assert not seen[r] and owner[r] == owner[s]
            seen[r] = True
        first, last = placed[0], placed[-1]
        ends = ((first[1], 1 if first[2] else 0), (last[1], 0 if last[2] else 1))
        peers = tuple(cross.get(e) for e in ends)
        frags.append({"rank": owner[s], "start": s, "key": strs[s], "placed": placed, "cyc": cyc, "ends": ends, "peers": peers,
                      "m": mrows, "sum": sum(counts[r] for _, r, _ in placed), "lp_start": next(p for p, r, _ in placed if r == s),
                      "open": peers[0] is not None or peers[1] is not None})
    per_rank = []
    for r in range(world):
        mine = [f for f in frags if f["rank"] == r]
        per_rank.append({"open": [f for f in mine if f["open"]], "closed": [f for f in mine if not f["open"]],
                         "local_cycles": sum(1 for f in mine if f["cyc"]),
                         "cross_links": sum(1 for p in cross if owner[p[0]] == r)})
        assert not any(f["cyc"] and f["open"] for f in mine)
    # the contigs: closed fragments, and the components of the open ones under their cross links
    opens = [f for f in frags if f["open"]]
    end_of = {e: (x, y) for x, f in enumerate(opens) for y, e in enumerate(f["ends"])}

    def fentry(x, y):
        p = opens[x]["peers"][y]
        q = end_of.get(p) if p is not None else None
        if q is None or opens[q[0]]["peers"][q[1]] != opens[x]["ends"][y]:
            return None
        return q

    def ftravel(x, y):
        out = [(x, y)]
        while fentry(x, y) is not None:
            x2, y2 = fentry(x, y)
            x, y = x2, y2 ^ 1
            if (x, y) == out[0]:
                return out, True
            out.append((x, y))
        return out, False

    contigs = [{"key": f["key"], "cyclic": f["cyc"], "rows": f["m"], "frags": [(f, 0, 0)], "rot": 0, "cross": False,
                "sum": f["sum"], "start": f["start"]} for f in frags if not f["open"]]
    fseen = [False] * len(opens)
    for x in range(len(opens)):
        if fseen[x]:
            continue
        left, cyc = ftravel(x, 0)
        members = [a for a, _ in left]
        if not cyc:
            members += [a for a, _ in ftravel(x, 1)[0][1:]]
        s = min(members, key=lambda a: opens[a]["key"])
        chain, cyc = ftravel(s, 0)
        order = [(a, 0 if y == 0 else 1) for a, y in reversed(chain)]  # left to right, the start fragment last
        if not cyc:
            order += [(a, 0 if y == 1 else 1) for a, y in ftravel(s, 1)[0][1:]]
        assert sorted(a for a, _ in order) == sorted(members)
        off, laid = 0, []
        for a, frc in order:
            fseen[a] = True
            laid.append((opens[a], frc, off))
            off += opens[a]["m"]
        rot = opens[s]["m"] - 1 - opens[s]["lp_start"] if cyc else 0
        contigs.append({"key": opens[s]["key"], "cyclic": cyc, "rows": off, "frags": laid, "rot": rot, "cross": True,
                        "sum": sum(opens[a]["sum"] for a, _ in order), "start": opens[s]["start"]})
    contigs.sort(key=lambda c: c["key"])
    return {"ranks": per_rank, "contigs": contigs, "frags": frags, "n_cross": sum(1 for c in contigs if c["cross"]),
            "cycles_cross": sum(1 for c in contigs if c["cross"] and c["cyclic"])}


def layout_ref(t: m.KmerTable, fr: dict) -> dict:
    """Stages 4 to 6: every row's contig (in start-key order over all contigs), position and strand, the contigs' bases,
    rows and depths, from the fragments' places alone."""
    n, k = len(t), t.k
    strs = m.keys_to_strings(t.keys, k) if n else []
    counts = [int(x) for x in t.counts]
    row_ctg = np.full(n, NO_ROW, dtype=np.uint32)
    row_pos = np.zeros(n, dtype=np.uint32)
    row_rc = np.zeros(n, dtype=np.uint8)
    seqs, depths, n_kmers = [], [], []
    for c, ctg in enumerate(fr["contigs"]):
        rows_total = ctg["rows"]
        at = [None] * rows_total
        for f, frc, off in ctg["frags"]:
            for lp, r, lrc in f["placed"]:
                p0 = off + (f["m"] - 1 - lp if frc else lp)
                pos = (p0 + ctg["rot"]) % rows_total if ctg["cyclic"] and ctg["cross"] else p0
                rc = lrc ^ frc
                assert at[pos] is None
                at[pos] = revcomp(strs[r]) if rc else strs[r]
                row_ctg[r], row_pos[r], row_rc[r] = c, pos, rc
        for a, b in zip(at, at[1:]):
            assert a[1:] == b[:-1], "neighbouring rows of a contig do not overlap"
        seqs.append("".join(o[0] for o in at[:-1]) + at[-1])
        depths.append((ctg["sum"] + counts[ctg["start"]]) / (rows_total + 1))
        n_kmers.append(rows_total)
    return {"row_ctg": row_ctg, "row_pos": row_pos, "row_rc": row_rc, "seqs": seqs,
            "depths": np.array(depths, dtype=np.float64), "n_kmers": np.array(n_kmers, dtype=np.uint32)}
