"""nh_build_db on the GPU (nohuman_amd/csrc/nh_build.hip): FASTA in, a kraken2 database directory out, against the Python model
of a one-taxon build (oracle/minidb.py build_hash) and then used as a database: nh_open's content check, a run with a calls
table, the CPU oracle, the CLI.

Which key sits in which occupied cell of a probe run depends on the order in which the waves arrive (as in kraken2's threaded
build), so tables are compared by header, occupied positions and sorted cells (tests/build_db_util.py same_table).  That is the
whole table only while no two distinct minimizers share a compacted key: build_db_util.order_free asserts it for every input
used here, on the CPU, before anything is compared.  Inputs that share keys on purpose: tests/test_gpu_build_db_forge.py."""
import os
import subprocess

import numpy as np
import pytest

from oracle import minidb
from tests import build_db_util as u
from tests import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "nohuman_amd", "bin", "nohuman")
BIG_PIECE = 1 << 30  # more k-mers than any sequence here: one piece a sequence
NH_EINVAL, NH_ECAPACITY = -1, -6


def build(paths, out_dir, **kw):
    import nohuman_amd
    return nohuman_amd.build_db(paths, str(out_dir), **kw)


def table(d):
    hdr, cells, _, _ = u.read_db(str(d))
    return hdr, cells


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    """the 20 kb genome, its model (computed once) and its default build on the GPU"""
    tmp = tmp_path_factory.mktemp("build_db")
    recs = u.genome(1)
    seqs = [s for _, s in recs]
    mins, kmers, amb = u.minimizers(seqs)
    cap = u.default_capacity(len(mins))
    model, size, _ = u.order_free(seqs, cap, mins)
    fa = u.write_fasta(tmp / "genome.fa", recs)
    out = tmp / "db"
    stats = build([fa], out)
    return dict(tmp=tmp, recs=recs, seqs=seqs, mins=mins, kmers=kmers, amb=amb, cap=cap, model=model, size=size, fa=fa, db=out,
                stats=stats)


def test_model_equivalence(ref):
    st = ref["stats"]
    hdr, cells, ob, _ = u.read_db(str(ref["db"]))
    assert st["distinct_minimizers"] == len(ref["mins"])
    assert st["capacity"] == ref["cap"] == u.default_capacity(len(ref["mins"]), 0.7) == hdr[0]
    assert st["size"] == ref["size"] == hdr[1] == int((cells != 0).sum())
    assert hdr[2:] == (30, 2)
    u.same_table((hdr, cells), u.cells_of(ref["model"]))
    assert st["sequences"] == len(ref["seqs"]) and st["bases"] == sum(len(s) for s in ref["seqs"])
    assert st["kmers"] == ref["kmers"] and st["ambiguous_kmers"] == ref["amb"]
    assert ob == minidb.opts_bytes()
    from oracle import oracle as orc
    odb = orc.OracleDB(directory=str(ref["db"]))
    assert odb.node_count == 3 and list(odb.external_ids) == [0, 1, 9606]
    assert set(os.listdir(ref["db"])) == set(u.DB_FILES)


def test_taxon_arguments(ref, tmp_path):
    """another taxon id and name: the same cells, the id and the name in taxo.k2d"""
    build([ref["fa"]], tmp_path / "db", taxid=10090, taxon_name="Mus musculus")
    hdr, cells, _, tb = u.read_db(str(tmp_path / "db"))
    u.same_table((hdr, cells), table(ref["db"]))
    from oracle import oracle as orc
    assert list(orc.OracleDB(directory=str(tmp_path / "db")).external_ids) == [0, 1, 10090]
    assert b"root\0Mus musculus\0" in tb and tb.endswith(b"no rank\0")
    build([ref["fa"]], tmp_path / "db2", taxid=10090)
    assert b"root\0taxon10090\0" in u.read_db(str(tmp_path / "db2"))[3]
    assert b"root\0Homo sapiens\0" in u.read_db(str(ref["db"]))[3]


@pytest.mark.parametrize("P", [64, 130])
def test_piece_borders(tmp_path, P):
    """pieces of 64 k-mers (less than a tile) and of 130 (more than one): the model, the build cut into pieces and the build
    with one piece a sequence give one table; a record again and its reverse complement add no cell"""
    recs = u.border_records(P)
    seqs = [s for _, s in recs]
    mins, kmers, amb = u.minimizers(seqs)
    cap = u.default_capacity(len(mins))
    model, size, _ = u.order_free(seqs, cap, mins)
    fa = u.write_fasta(tmp_path / "b.fa", recs)
    st_p = build([fa], tmp_path / "cut", piece_kmers=P)
    st_w = build([fa], tmp_path / "whole", piece_kmers=BIG_PIECE)
    for st in (st_p, st_w):
        assert (st["distinct_minimizers"], st["capacity"], st["size"]) == (len(mins), cap, size)
        assert (st["sequences"], st["kmers"], st["ambiguous_kmers"]) == (len(recs), kmers, amb)
    u.same_table(table(tmp_path / "cut"), u.cells_of(model))
    u.same_table(table(tmp_path / "whole"), u.cells_of(model))
    # the record without N or lowercase (the last of the length cases), again and as its reverse complement
    clean = recs[7][1]
    assert len(clean) == 2 * P + 34 and set(clean) <= set(b"ACGT")
    more = recs + [(b"again", clean), (b"revcomp", synth.revcomp(clean))]
    st_m = build([u.write_fasta(tmp_path / "m.fa", more)], tmp_path / "more", piece_kmers=P)
    assert (st_m["distinct_minimizers"], st_m["capacity"], st_m["size"]) == (len(mins), cap, size)
    assert st_m["kmers"] == kmers + 2 * (2 * P)
    u.same_table(table(tmp_path / "more"), u.cells_of(model))


def test_batch_borders(ref, tmp_path, monkeypatch):
    """the text goes to the device in batches: with batches of 1000 bytes every sequence is cut at the batches' ends as well"""
    monkeypatch.setenv("NOHUMAN_BUILD_BATCH", "1000")
    st = build([ref["fa"]], tmp_path / "db", piece_kmers=300)
    assert (st["distinct_minimizers"], st["size"], st["kmers"], st["ambiguous_kmers"]) == \
        (len(ref["mins"]), ref["size"], ref["kmers"], ref["amb"])
    u.same_table(table(tmp_path / "db"), u.cells_of(ref["model"]))


def test_the_counting_set_grows(tmp_path, monkeypatch):
    """300 kb in batches of 20 kb: the set of the counting pass starts at 65536 slots and is doubled (its keys re-inserted on the
    device) more than once on the way to some 100 000 minimizers; the build in one batch, whose set is sized once, gives the same
    count and the same table; the count is the C scanner's (no Python model at this size)."""
    rng = np.random.default_rng(5)
    recs = [(b"s%d" % i, synth.random_seq(rng, 100_000 + i)) for i in range(3)]
    mins = u.fast_minimizers([s for _, s in recs])
    u.assert_order_free_fast(mins, u.default_capacity(len(mins)), apart=1024)
    fa = u.write_fasta(tmp_path / "g.fa", recs)
    one = build([fa], tmp_path / "one")
    assert one["distinct_minimizers"] == len(mins) == one["size"] and one["capacity"] == u.default_capacity(len(mins))
    assert u.longest_run(table(tmp_path / "one")[1]) < 1024
    monkeypatch.setenv("NOHUMAN_BUILD_BATCH", "20000")
    many = build([fa], tmp_path / "many")
    assert one["distinct_minimizers"] > 2 * 65536 // 2 and one["kmers"] == sum(len(s) - 34 for _, s in recs)
    for k in ("sequences", "bases", "kmers", "ambiguous_kmers", "distinct_minimizers", "capacity", "size"):
        assert one[k] == many[k], k
    u.same_table(table(tmp_path / "one"), table(tmp_path / "many"))
    assert one["ambiguous_kmers"] == 0


def test_input_forms(ref, tmp_path):
    """wrapped at 60 columns with a short last line (the fixture), unwrapped, CRLF, gzip, two files, FASTQ: one table"""
    recs = ref["recs"]
    assert all(len(s) % 60 for _, s in recs)
    forms = {
        "unwrapped": [u.write_fasta(tmp_path / "u.fa", recs, width=0)],
        "crlf": [u.write_fasta(tmp_path / "c.fa", recs, crlf=True)],
        "gzip": [u.write_fasta(tmp_path / "g.fa.gz", recs, gz=True)],
        "two_files": [u.write_fasta(tmp_path / "t1.fa", recs[:3]), u.write_fasta(tmp_path / "t2.fa", recs[3:], width=71)],
    }
    fq = tmp_path / "q.fq"  # FASTQ is accepted: the reader yields its sequences
    fq.write_bytes(b"".join(b"@" + n + b"\n" + s + b"\n+\n" + b"I" * len(s) + b"\n" for n, s in recs))
    forms["fastq"] = [str(fq)]
    want = table(ref["db"])
    for name, paths in forms.items():
        st = build(paths, tmp_path / name, threads=2)
        assert (st["sequences"], st["bases"], st["distinct_minimizers"]) == \
            (ref["stats"]["sequences"], ref["stats"]["bases"], ref["stats"]["distinct_minimizers"]), name
        u.same_table(table(tmp_path / name), want)


def _reads(ref, n_genome=150, n_random=100):
    """FASTQ text: reads of 150 bases drawn from the genome, both strands, one to three substitutions each; random reads"""
    rng = np.random.default_rng(5)
    seqs = [s for s in ref["seqs"]]
    reads = []
    for i in range(n_genome):
        s = seqs[int(rng.integers(0, len(seqs)))]
        while True:
            p = int(rng.integers(0, len(s) - 150))
            r = bytearray(s[p:p + 150].upper())
            if b"N" not in r:
                break
        for q in rng.integers(0, 150, size=int(rng.integers(1, 4))):
            r[int(q)] = ord("ACGT"[(b"ACGT".index(r[int(q)]) + 1) % 4])
        r = bytes(r)
        reads.append((b"g%d" % i, synth.revcomp(r) if i % 2 else r, True))
    reads += [(b"r%d" % i, synth.random_seq(rng, 150), False) for i in range(n_random)]
    order = rng.permutation(len(reads))
    reads = [reads[int(i)] for i in order]
    text = b"".join(b"@" + n + b"\n" + s + b"\n+\n" + b"I" * len(s) + b"\n" for n, s, _ in reads)
    return reads, text


def test_it_is_a_database(ref, tmp_path):
    import nohuman_amd
    from nohuman_amd import engine
    from oracle import oracle as orc
    with nohuman_amd.Engine.open(str(ref["db"])) as eng:
        info = eng.info
        assert (info.capacity, info.size, info.key_bits, info.value_bits, info.node_count) == (ref["cap"], ref["size"], 30, 2, 3)
        assert eng.db_check().non_empty_cells == ref["size"] and eng.db_check().max_value == 2
        assert eng.external_id(2) == 9606
    reads, text = _reads(ref)
    fq = tmp_path / "reads.fq"
    fq.write_bytes(text)
    model_dir = tmp_path / "model_db"
    minidb.write_db(str(model_dir), minidb.opts_bytes(), u.taxonomy().to_bytes(), ref["model"])
    calls = {}
    for name, d in (("gpu", ref["db"]), ("model", model_dir)):
        o = tmp_path / name
        o.mkdir()
        st = engine.run(str(d), str(fq), str(o / "kept.fq"), calls=str(o / "calls.tsv"), report=str(o / "report.txt"), threads=2)
        calls[name] = (o / "calls.tsv").read_bytes()
        assert st.total_sequences == len(reads)
    assert calls["gpu"] == calls["model"]
    rows = [ln.split(b"\t") for ln in calls["gpu"].splitlines()]
    assert [r[1] for r in rows] == [n for n, _, _ in reads]
    for r, (n, _, from_genome) in zip(rows, reads):
        assert (r[0], r[2]) == ((b"C", b"9606") if from_genome else (b"U", b"0")), n
    odb = orc.OracleDB(directory=str(ref["db"]))
    odb.set(ambiguity_rule=u.rule())
    bases, offs = orc.pack_reads([s for _, s, _ in reads], False)
    exp, _ = odb.classify(bases, offs, False, 0.0)
    ext = odb.external_ids
    got = [(int(r[2]), int(r[4]), int(r[5]), int(r[6])) for r in rows]
    assert got == [(int(ext[int(e["call"])]), int(e["total_kmers"]), int(e["clade_hits"]), int(e["hit_groups"])) for e in exp]
    report = (tmp_path / "gpu" / "report.txt").read_bytes()
    assert b"Homo sapiens" in report and b"9606" in report
    kept = (tmp_path / "gpu" / "kept.fq").read_bytes()
    assert kept.count(b"\n") == 4 * sum(1 for r in reads if not r[2]) and b"@g" not in kept


def test_given_capacity(ref, tmp_path):
    """a capacity given: no counting pass, the model's table at that capacity; one too small: NH_ECAPACITY, no files, and the
    device builds on"""
    import nohuman_amd
    cap = 12007
    model, size, _ = u.order_free(ref["seqs"], cap, ref["mins"])
    st = build([ref["fa"]], tmp_path / "db", capacity=cap)
    assert st["distinct_minimizers"] == 0 and st["seconds_count"] == 0 and (st["capacity"], st["size"]) == (cap, size)
    assert (st["kmers"], st["ambiguous_kmers"]) == (ref["kmers"], ref["amb"])
    u.same_table(table(tmp_path / "db"), u.cells_of(model))
    for small in (len(ref["mins"]) // 2, len(ref["mins"])):  # (a table without an empty cell is refused as well)
        with pytest.raises(nohuman_amd.EngineError) as ei:
            build([ref["fa"]], tmp_path / "small", capacity=small)
        assert ei.value.code == NH_ECAPACITY and "capacity" in ei.value.message
        assert not (tmp_path / "small").exists()
    build([ref["fa"]], tmp_path / "after")
    u.same_table(table(tmp_path / "after"), table(ref["db"]))


def test_overwrite_and_rollback(ref, tmp_path):
    import nohuman_amd
    d = tmp_path / "db"
    build([ref["fa"]], d)
    old = {n: (d / n).read_bytes() for n in u.DB_FILES}
    other = u.write_fasta(tmp_path / "other.fa", u.genome(2, n_seq=2))
    with pytest.raises(nohuman_amd.EngineError) as ei:
        build([other], d)
    assert ei.value.code == NH_EINVAL and "force" in ei.value.message
    with pytest.raises(nohuman_amd.EngineError) as ei:  # a failed build: the old files stay, byte for byte, and nothing else
        build([other], d, capacity=100, force=True)
    assert ei.value.code == NH_ECAPACITY
    assert set(os.listdir(d)) == set(u.DB_FILES) and {n: (d / n).read_bytes() for n in u.DB_FILES} == old
    st = build([other], d, force=True, taxid=562)
    assert set(os.listdir(d)) == set(u.DB_FILES)
    hdr, cells, _, tb = u.read_db(str(d))
    assert hdr[0] == st["capacity"] != ref["cap"] and int((cells != 0).sum()) == st["size"]
    assert tb != old["taxo.k2d"]
    with nohuman_amd.Engine.open(str(d)) as eng:
        assert eng.external_id(2) == 562


def test_no_kmer_at_all(tmp_path):
    import nohuman_amd
    fa = u.write_fasta(tmp_path / "n.fa", [(b"short", b"ACGT" * 8), (b"all_n", b"N" * 500), (b"empty", b"")])
    for kw in (dict(), dict(capacity=1000)):
        with pytest.raises(nohuman_amd.EngineError) as ei:
            build([fa], tmp_path / "db", **kw)
        assert ei.value.code == -3 and "no k-mer" in ei.value.message  # NH_EDB
        assert not (tmp_path / "db").exists()
    with pytest.raises(nohuman_amd.EngineError) as ei:
        build([str(tmp_path / "missing.fa")], tmp_path / "db")
    assert ei.value.code == -2 and not (tmp_path / "db").exists()  # NH_EIO


def test_cli(ref, tmp_path):
    """nohuman --build-db on a FASTA, then nohuman --db on reads, end to end"""
    reads, text = _reads(ref, 60, 40)
    fq = tmp_path / "reads.fq"
    fq.write_bytes(text)
    d = tmp_path / "clidb"
    p = subprocess.run([BIN, "--build-db", str(d), "--reference", ref["fa"], "--taxid", "9606", "-t", "2"], capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode(errors="replace")
    err = p.stderr.decode(errors="replace")
    assert "%d distinct minimizers, capacity %d, size %d" % (len(ref["mins"]), ref["cap"], ref["size"]) in err, err
    u.same_table(table(d), table(ref["db"]))
    p = subprocess.run([BIN, "--build-db", str(d), "--reference", ref["fa"]], capture_output=True, timeout=300)
    assert p.returncode == 1 and b"force" in p.stderr
    out = tmp_path / "kept.fq"
    p = subprocess.run([BIN, "--db", str(d), str(fq), "-o", str(out)], capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode(errors="replace")
    assert "%d / %d" % (60, 100) in p.stderr.decode(errors="replace")
    kept = out.read_bytes()
    assert kept == b"".join(b"@" + n + b"\n" + s + b"\n+\n" + b"I" * len(s) + b"\n" for n, s, g in reads if not g)
