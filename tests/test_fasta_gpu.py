"""Assembly statistics and FASTA text of device-resident contigs on the GPU, one rank (mhmkc_ctgs_stats_device,
mhmkc_uutigs_stats, mhmkc_ctgs_fasta_device, mhmkc_uutigs_fasta, mhmkc_fasta_device / _fetch / _write / _info) against the
plain-Python reference of fasta_cases.py: the text byte for byte, the integer figures exactly, tot_depth within the bound
derived there and bit-equal on a second call."""
from __future__ import annotations

import ctypes as C
import struct

import numpy as np
import pytest

import fasta_cases as F
import mhm2_proxy_amd as m
from mhm2_proxy_amd import _native as N
from common import synth_set

pytestmark = pytest.mark.gpu

EINVAL, ESTATE, EUNSUPPORTED, EIO = -1, -5, -7, -9
INT_FIELDS = ("n_ctgs", "tot_len", "max_len", "n_ns", "len_sums", "n50", "l50")


def bits(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


@pytest.fixture(scope="module")
def counter():
    c = m.KmerCounter(21, device=0)  # the generic calls take a handle in any state
    yield c
    c.close()
    N.debug_reset()


def tensors(case, shift: int = 0):
    """The case's arrays on the device; shift: the bases start that many bytes into their allocation."""
    import torch

    bases, offsets, depths = F.arrays(case)
    big = torch.zeros(len(bases) + shift + 16, dtype=torch.uint8, device="cuda")
    seqs_t = big[shift:shift + len(bases)]
    seqs_t.copy_(torch.from_numpy(bases))
    return seqs_t, torch.from_numpy(offsets.view(np.int64)).cuda(), torch.from_numpy(depths).cuda()


def check_stats(c, case, min_len, got):
    exp = F.stats_ref(case.seqs, case.depths, min_len)
    assert got["mine"] == got["all"]  # one rank
    st = got["mine"]
    print(f"{case.name} min_len={min_len}: n_ctgs={st['n_ctgs']} tot_depth={st['tot_depth']!r} "
          f"fsum={exp['tot_depth']!r} err={abs(st['tot_depth'] - exp['tot_depth']):.3e} "
          f"bound={F.depth_bound([d for s, d in zip(case.seqs, case.depths) if len(s) >= min_len]):.3e}")
    for f in INT_FIELDS:
        assert st[f] == exp[f], (case.name, min_len, f)
    kept = [d for s, d in zip(case.seqs, case.depths) if len(s) >= min_len]
    assert abs(st["tot_depth"] - exp["tot_depth"]) <= F.depth_bound(kept)
    return st


def check_text(c, case, min_len, info):
    ref = F.fasta_ref(case.seqs, case.depths, case.first_id, min_len)
    assert info == {"n_bytes": len(ref), "file_offset": 0, "n_bytes_all": len(ref)}
    got = c.fasta_bytes()
    if got != ref:  # (name the first difference, not a megabyte of text)
        i = next(i for i, (a, b) in enumerate(zip(got, ref)) if a != b) if len(got) == len(ref) else -1
        raise AssertionError(f"{case.name} min_len={min_len}: text differs at byte {i}: "
                             f"{got[max(i - 40, 0):i + 40]!r} != {ref[max(i - 40, 0):i + 40]!r}")
    assert c.fasta_tensor().cpu().numpy().tobytes() == ref
    fi = c.fasta_info()
    assert fi["n_ctgs"] == len(case.seqs) and fi["n_written"] == ref.count(b">") and fi["n_bytes"] == len(ref)
    return ref


@pytest.mark.parametrize("case", F.all_cases(), ids=lambda c: c.name)
def test_text_and_stats_equal_the_reference(counter, case):
    c = counter
    seqs_t, offs_t, depths_t = tensors(case)
    for min_len in case.min_lens:
        check_text(c, case, min_len, c.ctgs_fasta_tensors(seqs_t, offs_t, depths_t, case.first_id, min_len))
        st = check_stats(c, case, min_len, c.ctgs_stats_tensors(seqs_t, offs_t, depths_t, min_len))
        again = c.ctgs_stats_tensors(seqs_t, offs_t, depths_t, min_len)["mine"]
        assert bits(again["tot_depth"]) == bits(st["tot_depth"]) and again == st


@pytest.mark.parametrize("shift,grid", [(0, 3), (1, 0), (7, 2), (15, 0), (8, 1)])
def test_unaligned_bases_and_strided_grids_change_nothing(counter, shift, grid):
    """The bases at every kind of offset into their 16-byte unit, and the kernels' grid-stride loops made to stride (the
    knob query_grid caps their grids): the same text, the same figures, the same tot_depth bits."""
    c = counter
    base = {}
    for case in (F.lengths_case(), F.ns_case()):
        s0, o0, d0 = tensors(case)
        base[case.name] = {mn: c.ctgs_stats_tensors(s0, o0, d0, mn)["mine"] for mn in case.min_lens}
    sd, od, dd = tensors(F.depths_case())
    deep = c.ctgs_stats_tensors(sd, od, dd, 0)["mine"]
    assert len(F.depths_case().seqs) > 14 * 1024
    try:
        N.debug_set("query_grid", grid)
        for case in (F.lengths_case(), F.ns_case()):
            seqs_t, offs_t, depths_t = tensors(case, shift)
            assert seqs_t.data_ptr() % 16 == shift
            for min_len in case.min_lens:
                check_text(c, case, min_len, c.ctgs_fasta_tensors(seqs_t, offs_t, depths_t, case.first_id, min_len))
                st = check_stats(c, case, min_len, c.ctgs_stats_tensors(seqs_t, offs_t, depths_t, min_len))
                assert bits(st["tot_depth"]) == bits(base[case.name][min_len]["tot_depth"])
        if grid:  # fifteen chunks of depths taken by one to three workgroups: the same sum, bit for bit
            assert bits(c.ctgs_stats_tensors(sd, od, dd, 0)["mine"]["tot_depth"]) == bits(deep["tot_depth"])
    finally:
        N.debug_reset()


@pytest.mark.parametrize("k", [21, 63, 99])
def test_uutigs_forms_equal_the_reference_on_uutigs(k):
    b, o = synth_set(3000, 20000, 5)
    c = m.KmerCounter(k, device=0)
    try:
        for turn in range(2):
            c.add_packed_reads(b, o)
            c.finish()
            plain = c.stats()["device_bytes"]
            offsets, seqs, depths, _ = c.uutigs()
            blob = seqs.tobytes()
            ctgs = tuple(blob[int(offsets[i]):int(offsets[i + 1])] for i in range(len(depths)))
            case = F.Case(f"uutigs-k{k}", ctgs, tuple(depths.tolist()), 0, (0, k + 20))
            assert len(ctgs) > 10 and any(len(s) < k + 20 for s in ctgs) and any(len(s) >= k + 20 for s in ctgs)
            built = c.stats()["device_bytes"]
            for min_len in case.min_lens:
                ref = check_text(c, case, min_len, c.uutigs_fasta(min_len))
                check_stats(c, case, min_len, c.uutigs_stats(min_len))
                held = c.stats()["device_bytes"]
                assert built + len(ref) <= held <= built + len(ref) + len(ref) // 16 + 8192  # the text, no scratch left
                assert c.fasta_info()["text_bytes"] == held - built
            c.reset()
            assert c.stats()["device_bytes"] == plain  # uutigs and text given back
            with pytest.raises(N.MhmkcError) as e:  # the kept text went with the round
                c.fasta_bytes()
            assert e.value.code == ESTATE
            if turn == 0:
                first = built - plain
            else:
                assert built - plain == first  # the second round's uutigs take what the first's took: no text is left
    finally:
        c.close()


def kinds_of(ref: bytes) -> bytes:
    """Per byte of a FASTA text: h header, s sequence, n a newline."""
    out, header = bytearray(), False
    for ch in ref:
        if ch == 0x3E:
            header = True
        out.append(ord("n") if ch == 0x0A else ord("h") if header else ord("s"))
        if ch == 0x0A:
            header = False
    return bytes(out)


def test_fasta_write_equals_the_text_at_every_chunk_size(counter, tmp_path):
    c = counter
    case = F.filter_case()
    seqs_t, offs_t, depths_t = tensors(case)
    c.ctgs_fasta_tensors(seqs_t, offs_t, depths_t, case.first_id, 0)
    ref = F.fasta_ref(case.seqs, case.depths, case.first_id, 0)
    kinds = kinds_of(ref)
    assert len(ref) > 4096 + 64
    try:
        for chunk in (64, 65, 4096, 0):
            if chunk in (64, 65):  # a chunk edge inside a header, inside a sequence and on a newline, from the offsets
                edges = {kinds[e:e + 1] for e in range(chunk, len(ref), chunk)}
                assert edges == {b"h", b"s", b"n"}, (chunk, edges)
            N.debug_set("fasta_chunk_bytes", chunk)
            path = tmp_path / f"out{chunk}.fasta"
            path.write_bytes(b"x" * (len(ref) + 100))  # an older, longer file is replaced
            c.fasta_write(path)
            assert path.read_bytes() == ref
            fi = c.fasta_info()
            assert fi["write_chunks"] == (-(-len(ref) // chunk) if chunk else 1) and fi["ms_write"] > 0
        # an empty text makes an empty file
        c.ctgs_fasta_tensors(seqs_t, offs_t, depths_t, case.first_id, 10**6)
        path = tmp_path / "none.fasta"
        path.write_bytes(b"old")
        c.fasta_write(path)
        assert path.read_bytes() == b""
    finally:
        N.debug_reset()


class FakeLowerRank:
    """A transport for rank 1 of 2 whose rank 0 exists only here: it reports no failure and a text of `n0` bytes."""

    def __init__(self, n0: int):
        self.n0, self.calls = n0, []
        self._ag = N.ALLGATHER_FN(self._allgather)
        self._a2a = N.ALLTOALLV_FN(lambda *a: 1)
        self.struct = N.MhmkcTransport(None, self._ag, self._a2a)

    def _allgather(self, _ctx, send, recv, nbytes):
        self.calls.append(int(nbytes))
        C.memmove(recv + nbytes, send, nbytes)
        lower = (C.c_uint64 * (nbytes // 8))()
        if nbytes == 16:  # mhmkc_ctgs_fasta_device: status, n_bytes
            lower[1] = self.n0
        C.memmove(recv, lower, nbytes)
        return 0


def test_block_written_above_4_gib_of_a_sparse_file(tmp_path):
    """file_offset above 2^32: the second rank of two (the first one stands in the transport) writes a few KB there."""
    n0 = 2**32 + 12345
    case = F.filter_case()
    ref = F.fasta_ref(case.seqs, case.depths, 7, 0)
    assert 4096 < len(ref) < 65536
    path = tmp_path / "sparse.fasta"
    try:
        with open(path, "wb") as f:  # what rank 0 does: the file at its full length
            f.truncate(n0 + len(ref))
    except OSError as e:
        pytest.skip(f"the file system refuses a file of {n0 + len(ref)} bytes: {e}")
    xp = FakeLowerRank(n0)
    c = m.KmerCounter(21, device=0, rank=1, n_ranks=2, output_owner=N.MHMKC_OWNER_MINIMIZER, transport=xp)
    try:
        seqs_t, offs_t, depths_t = tensors(case)
        info = c.ctgs_fasta_tensors(seqs_t, offs_t, depths_t, 7, 0)
        assert info == {"n_bytes": len(ref), "file_offset": n0, "n_bytes_all": n0 + len(ref)}
        N.debug_set("fasta_chunk_bytes", 100)
        c.fasta_write(path)
        assert xp.calls == [16, 8, 8]  # sizes; the barrier after the file is made; the final status
        with open(path, "rb") as f:
            f.seek(n0 - 4096)
            assert f.read(4096) == bytes(4096)
            assert f.read() == ref
    finally:
        N.debug_reset()
        c.close()


def small_case():
    rng = np.random.default_rng(5)
    return F.Case("small", tuple(F.rand_seq(rng, 20 + i) for i in range(6)), (1.0, 2.0, 3.0, 4.0, 5.0, 6.0), 0, (0,))


@pytest.mark.parametrize("bad", [-1.5, -0.0, float("nan"), float("inf"), 2.0**32], ids=repr)
def test_unsupported_depths_are_refused_before_anything_is_written(counter, bad):
    c = counter
    case = small_case()
    seqs_t, offs_t, depths_t = tensors(case)
    c.ctgs_fasta_tensors(seqs_t, offs_t, depths_t, 0, 0)  # a text that the failing call must not leave behind
    depths_t[3] = bad
    depths_t[5] = bad
    with pytest.raises(N.MhmkcError) as e:
        c.ctgs_fasta_tensors(seqs_t, offs_t, depths_t, 0, 0)
    assert e.value.code == EINVAL and "contig 3 " in str(e.value)
    with pytest.raises(N.MhmkcError) as e:
        c.fasta_bytes()
    assert e.value.code == ESTATE
    # a contig that is not written is not formatted: its depth is not looked at
    info = c.ctgs_fasta_tensors(seqs_t, offs_t, depths_t, 0, 26)
    assert info["n_bytes"] == 0 and c.fasta_bytes() == b""


def test_id_overflow_and_bad_offsets_are_refused(counter, tmp_path):
    c = counter
    case = small_case()
    seqs_t, offs_t, depths_t = tensors(case)
    n = len(case.seqs)
    assert c.ctgs_fasta_tensors(seqs_t, offs_t, depths_t, F.ID_MAX - n, 0)["n_bytes"] > 0  # the bound itself
    for first in (F.ID_MAX - n + 1, F.ID_MAX, 2**63, 2**64 - 1):
        with pytest.raises(N.MhmkcError) as e:
            c.ctgs_fasta_tensors(seqs_t, offs_t, depths_t, first, 0)
        assert e.value.code == EINVAL and "2^63" in str(e.value)
    fall = offs_t.clone()
    fall[2], fall[3] = offs_t[3], offs_t[2]  # offsets that fall at contig 2
    start = offs_t.clone()
    start[0] = 1
    for bad_offs, name in ((fall, "contig 2"), (start, "contig 0")):
        for call in (lambda: c.ctgs_fasta_tensors(seqs_t, bad_offs, depths_t, 0, 0),
                     lambda: c.ctgs_stats_tensors(seqs_t, bad_offs, depths_t, 0)):
            with pytest.raises(N.MhmkcError) as e:
                call()
            assert e.value.code == EINVAL and name in str(e.value)
    with pytest.raises(N.MhmkcError) as e:
        c.fasta_write(tmp_path / "never.fasta")
    assert e.value.code == ESTATE and not (tmp_path / "never.fasta").exists()


def test_state_and_io_refusals(tmp_path):
    c = m.KmerCounter(21, device=0)
    try:
        for call in (c.fasta_bytes, c.fasta_tensor, lambda: c.fasta_write(tmp_path / "x.fasta")):
            with pytest.raises(N.MhmkcError) as e:
                call()
            assert e.value.code == ESTATE
        for call in (c.uutigs_stats, c.uutigs_fasta):  # the uutigs forms need a finished round
            with pytest.raises(N.MhmkcError) as e:
                call()
            assert e.value.code == ESTATE
        case = small_case()
        c.ctgs_fasta_tensors(*tensors(case), 0, 0)
        with pytest.raises(N.MhmkcError) as e:
            c.fasta_write(tmp_path / "no-such-dir" / "x.fasta")
        assert e.value.code == EIO and "No such file or directory" in str(e.value)
        c.fasta_write(tmp_path / "x.fasta")  # the text is still there
        assert (tmp_path / "x.fasta").read_bytes() == F.fasta_ref(case.seqs, case.depths, 0, 0)
    finally:
        c.close()


def test_uutigs_forms_refuse_a_multirank_handle_without_a_ranks_build():
    """MHMKC_EUNSUPPORTED before any collective (the handle has no transport: a collective would be MHMKC_ETRANSPORT)."""
    L = N.lib()
    cfg = N.MhmkcConfig()
    L.mhmkc_config_init(C.byref(cfg))
    cfg.n_ranks, cfg.rank, cfg.output_owner = 2, 0, N.MHMKC_OWNER_MINIMIZER
    h = C.c_void_p()
    assert L.mhmkc_create(C.byref(h), C.byref(cfg)) == 0
    try:
        assert L.mhmkc_uutigs_stats(h, 0, None, None) == EUNSUPPORTED
        assert L.mhmkc_uutigs_fasta(h, 0, None, None, None) == EUNSUPPORTED
    finally:
        L.mhmkc_destroy(h)
