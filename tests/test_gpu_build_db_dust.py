"""nh_build_db with mask_low_complexity on the GPU: the database of a genome with planted low-complexity stretches equals the
existing model of a build (tests/build_db_util.py) run on the sequences as tests/dust_model.py masks them, whatever the cuts into
pieces and batches; without the flag nothing changes; and a read that carries a microsatellite of the genome is kept with the
masked database and removed with the unmasked one."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import build_db_util as u
from tests import dust_model as dm
from tests import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "nohuman_amd", "bin", "nohuman")
SATELLITE = b"AC" * 30 + b"CAG" * 20 + b"AATGG" * 12  # 180 bases, in chr2 of the genome and in the read of test_end_to_end
COUNTS = ("sequences", "bases", "kmers", "ambiguous_kmers", "distinct_minimizers", "capacity", "size", "masked_bases")


def build(paths, out_dir, **kw):
    import nohuman_amd
    return nohuman_amd.build_db(paths, str(out_dir), **kw)


def table(d):
    hdr, cells, _, _ = u.read_db(str(d))
    return hdr, cells


def low_complexity_genome(seed=7):
    """u.genome(seed) with low-complexity stretches planted: at the very ends of records, next to N, longer than 64, shorter than
    7; and two records too short for a k-mer"""
    rng = np.random.default_rng(seed)
    recs = [(n, bytearray(s)) for n, s in u.genome(seed)]

    def put(i, pos, s):
        recs[i][1][pos:pos + len(s)] = s

    put(0, 0, b"T" * 30)                                   # the very start of a record
    put(0, len(recs[0][1]) - 45, dm.periodic(rng, 45, 2))  # and its very end
    put(0, 700, b"A" * 6)                                  # shorter than 7: not masked
    put(0, 900, b"G" * 5)
    put(1, 400, SATELLITE)
    put(1, 1500, b"N" + dm.periodic(rng, 70, 3) + b"N")    # next to N on both sides
    put(1, 2000, b"C" * 7)
    put(2, 1000, dm.biased(rng, 150))
    put(2, 2100, dm.periodic(rng, 300, 7))                 # longer than 64 by far
    put(3, 1090, b"A" * 40)                                # right behind the N run of u.genome's fourth record
    put(4, 300, dm.periodic(rng, 66, 4).lower())           # lowercase
    put(5, 1234, dm.periodic(rng, 63, 5))
    put(6, len(recs[6][1]) - 7, b"G" * 7)                  # 7 bases at the very end
    put(7, 0, dm.periodic(rng, 12, 2))
    out = [(n, bytes(s)) for n, s in recs]
    out += [(b"short_a", b"A" * 20), (b"short_mixed", b"ACGTTGCA" + b"T" * 9 + b"GGCATCA"), (b"tiny", b"AAAAAA")]
    return out


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    """the genome, the model of its masked build (computed once), its masked and its unmasked build on the GPU"""
    tmp = tmp_path_factory.mktemp("build_db_dust")
    recs = low_complexity_genome()
    seqs = [s for _, s in recs]
    masked_seqs = [dm.mask(s) for s in seqs]
    n_masked = sum(dm.masked_count(s) for s in seqs)
    total = sum(len(s) for s in seqs)
    assert 0.03 * total < n_masked < 0.2 * total  # (on the CPU, before any build: the masks are neither empty nor everything)
    assert masked_seqs[0][:30] == b"N" * 30 and masked_seqs[0][700:706] == b"A" * 6 and masked_seqs[-3] == b"N" * 20
    mins, kmers, amb = u.minimizers(masked_seqs)
    cap = u.default_capacity(len(mins))
    model, size, _ = u.order_free(masked_seqs, cap, mins)
    fa = u.write_fasta(tmp / "genome.fa", recs)
    fa_masked = u.write_fasta(tmp / "genome_masked.fa", list(zip([n for n, _ in recs], masked_seqs)))
    st = build([fa], tmp / "db", mask_low_complexity=True)
    st_plain = build([fa], tmp / "db_plain")
    return dict(tmp=tmp, recs=recs, seqs=seqs, masked_seqs=masked_seqs, n_masked=n_masked, mins=mins, kmers=kmers, amb=amb, cap=cap,
                model=model, size=size, fa=fa, fa_masked=fa_masked, db=tmp / "db", db_plain=tmp / "db_plain", stats=st,
                stats_plain=st_plain)


def assert_is_the_model(st, d, ref):
    assert (st["distinct_minimizers"], st["capacity"], st["size"]) == (len(ref["mins"]), ref["cap"], ref["size"])
    assert (st["sequences"], st["bases"]) == (len(ref["seqs"]), sum(len(s) for s in ref["seqs"]))
    assert (st["kmers"], st["ambiguous_kmers"]) == (ref["kmers"], ref["amb"])
    assert st["masked_bases"] == ref["n_masked"]
    u.same_table(table(d), u.cells_of(ref["model"]))


def test_model_equivalence(ref):
    assert_is_the_model(ref["stats"], ref["db"], ref)
    assert ref["stats"]["seconds_mask"] > 0
    # the unmasked build of the FASTA the model masked: the same database
    st = build([ref["fa_masked"]], ref["tmp"] / "db_of_masked")
    for k in COUNTS[:-1]:
        assert st[k] == ref["stats"][k], k
    assert st["masked_bases"] == 0 and st["seconds_mask"] == 0
    u.same_table(table(ref["tmp"] / "db_of_masked"), table(ref["db"]))
    # and the masking took minimizers out: without this the comparisons above would show nothing
    assert ref["stats"]["size"] < ref["stats_plain"]["size"]
    assert ref["stats"]["ambiguous_kmers"] > ref["stats_plain"]["ambiguous_kmers"]
    assert ref["stats_plain"]["masked_bases"] == 0


@pytest.mark.parametrize("P", [64, 130])
def test_pieces_do_not_matter(ref, tmp_path, P):
    assert_is_the_model(build([ref["fa"]], tmp_path / "db", mask_low_complexity=True, piece_kmers=P), tmp_path / "db", ref)


@pytest.mark.parametrize("batch", [1000, 997, 64])
def test_batches_do_not_matter(ref, tmp_path, monkeypatch, batch):
    """sequences cut at the batches' ends: stretches straddle the cuts, each chunk carries 63 bases of context (fewer at a
    sequence's ends), and every base is counted once"""
    monkeypatch.setenv("NOHUMAN_BUILD_BATCH", str(batch))
    assert_is_the_model(build([ref["fa"]], tmp_path / "db", mask_low_complexity=True, piece_kmers=300), tmp_path / "db", ref)
    assert_is_the_model(build([ref["fa"]], tmp_path / "db2", mask_low_complexity=True, capacity=ref["cap"]) |
                        {"distinct_minimizers": len(ref["mins"])}, tmp_path / "db2", ref)


def test_masking_off_is_the_build_as_it_was(ref, tmp_path):
    from nohuman_amd import _lib
    st = build([ref["fa"]], tmp_path / "off", mask_low_complexity=False)
    for k in COUNTS:
        assert st[k] == ref["stats_plain"][k], k
    assert st["seconds_mask"] == 0
    off = table(tmp_path / "off")
    u.same_table(off, table(ref["db_plain"]))
    # a caller of the first layout: struct_size 80, a stats buffer of 88 bytes -- here with a poisoned tail behind it
    assert C.sizeof(_lib.nh_build_args) == 80 and C.sizeof(_lib.nh_build_stats) == 88
    a = _lib.nh_build_args_v2()
    a.struct_size = C.sizeof(_lib.nh_build_args)
    a.mask_low_complexity = 1  # (behind the size the caller states: not read)
    paths = (C.c_char_p * 1)(os.fsencode(ref["fa"]))
    a.n_fasta, a.fasta, a.out_dir = 1, paths, os.fsencode(str(tmp_path / "old_caller"))
    s = _lib.nh_build_stats_v2()
    C.memset(C.byref(s), 0xA5, C.sizeof(s))
    assert _lib.lib().nh_build_db(C.byref(a), C.byref(s)) == 0, _lib.lib().nh_last_error()
    assert bytes(s)[88:] == b"\xa5" * 16
    assert (s.sequences, s.bases, s.kmers, s.size, s.capacity) == tuple(st[k] for k in ("sequences", "bases", "kmers", "size", "capacity"))
    u.same_table(table(tmp_path / "old_caller"), off)
    # the same caller with the present size: masked
    a.struct_size = C.sizeof(_lib.nh_build_args_v2)
    a.force = 1
    assert _lib.lib().nh_build_db(C.byref(a), C.byref(s)) == 0, _lib.lib().nh_last_error()
    assert s.masked_bases == ref["n_masked"] and s.size == ref["size"]


def satellite_read():
    rng = np.random.default_rng(99)
    return synth.random_seq(rng, 45) + SATELLITE[20:140] + synth.random_seq(rng, 45)


def test_end_to_end(ref, tmp_path):
    """a microbial read with a microsatellite of the genome between flanks the genome does not have: removed as human with the
    unmasked database, kept with the masked one"""
    from nohuman_amd import engine
    read = satellite_read()
    assert SATELLITE in ref["seqs"][1] and dm.mask(ref["seqs"][1])[400:580] == b"N" * 180
    # on the CPU first: the read's minimizers meet the unmasked genome's in more than two places and the masked genome's nowhere
    read_mins, _, _ = u.minimizers([read])
    plain_mins, _, _ = u.minimizers([ref["seqs"][1][300:700]])
    assert len(read_mins & plain_mins) >= 3 and not (read_mins & ref["mins"])
    fq = tmp_path / "reads.fq"
    other = synth.random_seq(np.random.default_rng(5), 150)
    fq.write_bytes(b"@satellite\n" + read + b"\n+\n" + b"I" * len(read) + b"\n@other\n" + other + b"\n+\n" + b"I" * 150 + b"\n")
    kept = {}
    for name, d in (("masked", ref["db"]), ("plain", ref["db_plain"])):
        out = tmp_path / (name + ".fq")
        engine.run(str(d), str(fq), str(out), threads=1)
        kept[name] = out.read_bytes()
    assert b"@satellite\n" in kept["masked"] and b"@other\n" in kept["masked"]
    assert b"@satellite\n" not in kept["plain"] and b"@other\n" in kept["plain"]


def test_cli(ref, tmp_path):
    d = tmp_path / "clidb"
    p = subprocess.run([BIN, "--build-db", str(d), "--reference", ref["fa"], "--mask-low-complexity"], capture_output=True, timeout=300)
    err = p.stderr.decode(errors="replace")
    assert p.returncode == 0, err
    assert "%d distinct minimizers, capacity %d, size %d" % (len(ref["mins"]), ref["cap"], ref["size"]) in err, err
    share = 100.0 * ref["n_masked"] / sum(len(s) for s in ref["seqs"])
    assert "%d low-complexity bases masked (%.2f %% of the bases)" % (ref["n_masked"], share) in err, err
    u.same_table(table(d), table(ref["db"]))
    p = subprocess.run([BIN, "--build-db", str(tmp_path / "plain"), "--reference", ref["fa"]], capture_output=True, timeout=300)
    assert p.returncode == 0 and b"low-complexity" not in p.stderr
    u.same_table(table(tmp_path / "plain"), table(ref["db_plain"]))
