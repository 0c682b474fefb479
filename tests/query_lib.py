"""Helpers of the query tests (test_query.py, test_dbjg_links.py): vectorised k-mer packing, the expected answers of
a lookup from a fetched table, the link rules of mhmkc_dbjg_links restated over a KmerTable, and a walker that
assembles uutigs from the links alone."""
from __future__ import annotations

import numpy as np

import mhm2_proxy_amd as m

NO_ROW = 0xFFFFFFFF
OK, DEADEND, FORK, CONFLICT, RC = 0, 1, 2, 3, 0x80
COMP = str.maketrans("ACGT", "TGCA")


def unpack_codes(keys: np.ndarray, k: int) -> np.ndarray:
    """(n, n_longs) uint64 keys -> (n, k) uint8 base codes (A0 C1 G2 T3)."""
    keys = np.asarray(keys, dtype=np.uint64)
    out = np.empty((keys.shape[0], k), dtype=np.uint8)
    for i in range(k):
        out[:, i] = ((keys[:, i // 32] >> np.uint64(2 * (31 - i % 32))) & np.uint64(3)).astype(np.uint8)
    return out


def pack_codes(codes: np.ndarray, n_longs: int) -> np.ndarray:
    """(n, k) base codes -> (n, n_longs) uint64 keys in Kmer::longs layout (the unused bits zero)."""
    n, k = codes.shape
    keys = np.zeros((n, n_longs), dtype=np.uint64)
    for i in range(k):
        keys[:, i // 32] |= codes[:, i].astype(np.uint64) << np.uint64(2 * (31 - i % 32))
    return keys


def revcomp_keys(keys: np.ndarray, k: int) -> np.ndarray:
    c = unpack_codes(keys, k)
    return pack_codes((3 - c[:, ::-1]).astype(np.uint8), keys.shape[1])


def mutate_keys(keys: np.ndarray, k: int, rng) -> np.ndarray:
    """Every key with one base (a random position) changed to another base."""
    c = unpack_codes(keys, k)
    n = c.shape[0]
    pos = rng.integers(0, k, size=n)
    c[np.arange(n), pos] = (c[np.arange(n), pos] + rng.integers(1, 4, size=n)) % 4
    return pack_codes(c.astype(np.uint8), keys.shape[1])


def row_dict(t: m.KmerTable) -> dict:
    return {t.keys[i].tobytes(): i for i in range(len(t))}


def expected_lookup(t: m.KmerTable, d: dict, q: np.ndarray, canonicalize: bool = False):
    """The answers of lookup(q) read from the fetched table through a Python dict of its rows."""
    q = np.ascontiguousarray(q, dtype=np.uint64)
    if canonicalize:
        rc = revcomp_keys(q, t.k)
        less = np.zeros(q.shape[0], dtype=bool)
        decided = np.zeros(q.shape[0], dtype=bool)
        for w in range(q.shape[1]):
            less |= ~decided & (rc[:, w] < q[:, w])
            decided |= rc[:, w] != q[:, w]
        q = np.where(less[:, None], rc, q)
        q = np.ascontiguousarray(q)
    rows = np.array([d.get(q[i].tobytes(), NO_ROW) for i in range(q.shape[0])], dtype=np.uint32).reshape(-1)
    hit = rows != NO_ROW
    safe = np.where(hit, rows, 0).astype(np.intp)
    if len(t) == 0:
        z = np.zeros(q.shape[0], dtype=np.uint8)
        return rows, z.astype(np.uint16), z, z
    counts = np.where(hit, t.counts[safe], 0).astype(np.uint16)
    left = np.where(hit, t.left[safe], 0).astype(np.uint8)
    right = np.where(hit, t.right[safe], 0).astype(np.uint8)
    return rows, counts, left, right


def assert_lookup(got, exp, what=""):
    for name, g, e in zip(("rows", "counts", "left", "right"), got, exp):
        g, e = np.asarray(g), np.asarray(e)
        assert g.shape == e.shape, f"{what}: {name} shape {g.shape} vs {e.shape}"
        bad = np.flatnonzero(g != e)
        i = int(bad[0]) if bad.size else 0
        assert bad.size == 0, f"{what}: {name} differs at {bad.size} queries, first {i}: {g[i]} vs {e[i]}"


# the cases of the link rules, for the coverage assertions
WHY = ("ok", "ok_rc", "dead_missing", "dead_own_x", "dead_nb_x", "fork_own", "fork_nb", "conflict")


def links_ref(t: m.KmerTable):
    """mhmkc_dbjg_links restated (include/mhmkc.h): next[2, n], status[2, n], why[2, n] (index into WHY)."""
    n = len(t)
    strs = m.keys_to_strings(t.keys, t.k) if n else []
    idx = {s: i for i, s in enumerate(strs)}
    ext = [(chr(int(t.left[i])), chr(int(t.right[i]))) for i in range(n)]
    nxt = np.full((2, n), NO_ROW, dtype=np.uint32)
    status = np.zeros((2, n), dtype=np.uint8)
    why = np.zeros((2, n), dtype=np.uint8)
    for d in (0, 1):
        for i, s in enumerate(strs):
            l, r = ext[i]
            if "X" in (l, r):
                status[d, i], why[d, i] = DEADEND, 3
                continue
            if "F" in (l, r):
                status[d, i], why[d, i] = FORK, 5
                continue
            nb = s[1:] + r if d else l + s[:-1]
            rc = nb[::-1].translate(COMP)
            is_rc = rc < nb
            j = idx.get(rc if is_rc else nb)
            if j is None:
                status[d, i], why[d, i] = DEADEND, 2
                continue
            nxt[d, i] = j
            jl, jr = ext[j]
            if "X" in (jl, jr):
                status[d, i], why[d, i] = DEADEND, 4
            elif "F" in (jl, jr):
                status[d, i], why[d, i] = FORK, 6
            else:
                if is_rc:
                    jl, jr = jr.translate(COMP), jl.translate(COMP)
                if (jl == s[0]) if d else (jr == s[-1]):
                    status[d, i], why[d, i] = (OK | RC, 1) if is_rc else (OK, 0)
                else:
                    status[d, i], why[d, i] = CONFLICT, 7
    return nxt, status, why


def walk_links(t: m.KmerTable, nxt: np.ndarray, status: np.ndarray) -> list:
    """The traversal of include/mhmkc_dbjg.hpp (lines 70-137) over the links alone: no k-mer is hashed or looked up,
    the bases come from the rows' extensions. Returns sorted "<canonical uutig> <depth %.6f>" lines, as
    tests/cpp/dbjg_test.cpp prints them."""
    n, k = len(t), t.k
    order = np.lexsort(tuple(t.keys[:, w] for w in range(t.keys.shape[1] - 1, -1, -1))) if n else []
    left = [chr(int(x)) for x in t.left]
    right = [chr(int(x)) for x in t.right]
    counts = t.counts.astype(np.int64)
    visited = np.full(n, -1, dtype=np.int64)
    lines = []
    n_walks = 0
    for start in order:
        start = int(start)
        if visited[start] >= 0 or left[start] not in "ACGT" or right[start] not in "ACGT":
            continue
        walk_id = n_walks
        n_walks += 1
        s = m.keys_to_strings(t.keys[start:start + 1], k)[0]
        uutig, sum_depths = "", 0
        for dirn in (0, 1):  # LEFT, then RIGHT (the start is visited by both: revisiting it is allowed once)
            row, d = start, dirn  # d: the direction in row's stored frame (flipped by every RC link)
            walk = [s[0]] if dirn == 0 else [s[1:k - 1], s[-1]]
            visited[start] = walk_id
            sum_depths += int(counts[start])
            while True:
                # the base this step adds: row's extension towards the walk, in the walk's frame
                if d == dirn:
                    ext = left[row] if dirn == 0 else right[row]
                else:
                    ext = (right[row] if dirn == 0 else left[row]).translate(COMP)
                st = int(status[d, row])
                if (st & ~RC) != OK:
                    break
                j = int(nxt[d, row])
                if visited[j] >= 0:  # REPEAT (this walk) or VISITED (another walk's k-mer)
                    break
                visited[j] = walk_id
                walk.append(ext)
                sum_depths += int(counts[j])
                row = j
                if st & RC:
                    d ^= 1
            part = "".join(walk)
            uutig += part[::-1] if dirn == 0 else part
        if len(uutig) < k:
            continue
        canon = min(uutig, uutig[::-1].translate(COMP))
        lines.append(f"{canon} {sum_depths / (len(uutig) - k + 2):.6f}")
    return sorted(lines)
