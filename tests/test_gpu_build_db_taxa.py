"""nh_build_db with a taxa manifest on the GPU: several taxa in one database, a minimizer of two taxa stored as their lowest common
ancestor.  Every table is compared with the Python model's (oracle/minidb.py build_hash) of the same (taxon, record) pairs; the
inputs are order free under the model (tests/test_build_taxa_model.py asserts it on the CPU), so the comparison leaves nothing
out: header, occupied positions and sorted cells.  Where keys are shared on purpose (build_forge.shared_key_records) the table of
sequential batches equals the model's cell for cell."""
import os
import subprocess

import numpy as np
import pytest

from oracle import minidb
from tests import build_db_util as u
from tests import build_forge as bf
from tests import build_taxa_util as t
from tests import dust_model as dm
from tests import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "nohuman_amd", "bin", "nohuman")


def build(taxa, out_dir, batch=None, **kw):
    import nohuman_amd
    with pytest.MonkeyPatch.context() as mp:
        if batch is None:
            mp.delenv("NOHUMAN_BUILD_BATCH", raising=False)
        else:
            mp.setenv("NOHUMAN_BUILD_BATCH", str(batch))
        return nohuman_amd.build_db(None, str(out_dir), taxa=taxa, **kw)


def table(d):
    hdr, cells, _, _ = u.read_db(str(d))
    return hdr, cells


def assert_is_the_model(st, d, c, counted=True):
    """the database in d and the stats of its build against the case's model"""
    tax = c["tax"]
    vb = minidb.value_bits_for(tax.node_count)
    hdr, cells, ob, tb = u.read_db(str(d))
    mhdr, mcells = u.cells_of(c["model"])
    assert hdr == mhdr == (c["cap"], c["size"], 32 - vb, vb)
    u.same_table((hdr, cells), (mhdr, mcells))
    assert ob == minidb.opts_bytes()
    assert t.parse_taxo(tb) == t.model_nodes(tax)
    assert (st["capacity"], st["size"], st["taxa"]) == (c["cap"], c["size"], tax.node_count - 1)
    if counted:
        assert st["distinct_minimizers"] == len(c["mins"])
    seqs = [s for _, s in c["pairs"]]
    assert (st["sequences"], st["bases"], st["kmers"]) == (len(seqs), sum(map(len, seqs)), sum(max(0, len(s) - 34) for s in seqs))
    counts = t.value_counts(mcells, vb, tax.node_count)
    per = t.per_taxon(c["pairs"], tax)
    ts = st["taxon_stats"]
    assert len(ts) == tax.node_count - 1
    assert [x["taxid"] for x in ts] == tax.external[1:]
    assert [x["cells"] for x in ts] == counts[1:] and sum(x["cells"] for x in ts) == st["size"]
    assert [(x["sequences"], x["bases"], x["kmers"]) for x in ts] == per[1:]


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """test 1's database: A, B under G under the root, C under the root, G with sequences of its own"""
    tmp = tmp_path_factory.mktemp("taxa_tree")
    c = t.tree_case()
    m = t.write_case(tmp, c["lines"], c["records"])
    st = build(m, tmp / "db")
    return dict(c, tmp=tmp, manifest=m, db=tmp / "db", stats=st)


def test_tree_and_lca(tree):
    assert_is_the_model(tree["stats"], tree["db"], tree)
    hdr, cells = table(tree["db"])
    assert hdr[2:] == (29, 3)
    counts = t.value_counts(cells, 3, 6)
    assert min(counts[1:]) > 0  # every node holds cells, the inner node and the root among them
    assert [n[4] for n in t.parse_taxo(u.read_db(str(tree["db"]))[3])] == ["root", "root", "taxon C", "group G", "taxon A", "taxon B"]
    # the same database from a capacity given (no counting pass) and from small pieces
    st = build(tree["manifest"], tree["tmp"] / "db_cap", capacity=tree["cap"], piece_kmers=130)
    assert st["distinct_minimizers"] == 0
    assert_is_the_model(st, tree["tmp"] / "db_cap", tree, counted=False)


@pytest.mark.parametrize("taxa", [(t.A, t.B, t.C_), (t.A, t.B)])
def test_races(tmp_path, taxa):
    """the same 20 kb under several taxa in pieces of 64 k-mers and one batch: about a thousand waves merge into the same cells
    in one launch.  Every cell ends at the lowest common ancestor of all the taxa, none at a leaf"""
    recs = t.race_records()
    tax = t.taxonomy_of(t.TREE_LINES)
    records = {x: recs for x in taxa}
    m = t.write_case(tmp_path, t.TREE_LINES, records)
    mins = u.fast_minimizers([s for _, s in recs])
    assert sum((len(s) - 34 + 63) // 64 for _, s in recs) * len(taxa) > 600  # pieces, a wave each
    st = build(m, tmp_path / "db", piece_kmers=64)
    hdr, cells = table(tmp_path / "db")
    want = tax.internal[t.G] if len(taxa) == 2 else 1
    assert st["size"] == len(mins) == hdr[1] == int((cells != 0).sum())
    values = np.unique(cells[cells != 0] & np.uint32(7)).tolist()
    assert values == [want], values
    assert [x["cells"] for x in st["taxon_stats"]] == [len(mins) if i + 1 == want else 0 for i in range(5)]
    one, _ = t.model(tax, [(taxa[0], s) for _, s in recs], st["capacity"])
    assert np.array_equal(np.sort(cells >> np.uint32(3)), np.sort(u.cells_of(one)[1] >> np.uint32(3)))  # the keys of one copy


@pytest.mark.parametrize("batch,P", [(997, 64), (997, 130), (64, 64), (64, 130)])
def test_borders(tmp_path, batch, P):
    """small batches: the last piece of one taxon and the first of the next in one batch, sequences cut at the batches' ends that go
    on under their own taxon, records shorter than 35 bases between the taxa"""
    c = t.border_case()
    m = t.write_case(tmp_path, c["lines"], c["records"])
    seqs = [s for _, s in c["pairs"]]
    cuts = bf.batches_of(seqs, batch)
    owner = [x for x, _ in c["pairs"]]
    assert any(len({owner[i] for i, _ in b}) > 1 for b in cuts) or batch == 64  # two taxa in one batch
    assert sum(1 for a, b in zip(cuts, cuts[1:]) if a[-1][0] == b[0][0]) > 5       # sequences that go on in the next batch
    assert any(len(s) < 35 for s in seqs)
    assert_is_the_model(build(m, tmp_path / "db", batch=batch, piece_kmers=P), tmp_path / "db", c)


def test_with_mask_low_complexity(tmp_path):
    """the table of a masked build of several taxa is the model's on the sequences as tests/dust_model.py masks them"""
    c = t.border_case()
    rng = np.random.default_rng(5)
    records = {x: list(r) for x, r in c["records"].items()}
    for x, i, at, s in ((t.A, 1, 200, dm.periodic(rng, 120, 2)), (t.B, 1, 1000, b"A" * 50), (t.C_, 0, 0, dm.periodic(rng, 70, 3)),
                        (t.G, 1, 1800, dm.periodic(rng, 90, 5)), (t.B, 2, 77, b"CAG" * 30)):
        n, seq = records[x][i]
        records[x][i] = (n, seq[:at] + s + seq[at + len(s):])
    tax = c["tax"]
    pairs = t.pairs_of(tax, records)
    masked = [(x, dm.mask(s)) for x, s in pairs]
    n_masked = sum(dm.masked_count(s) for _, s in pairs)
    assert n_masked > 400
    mins = u.fast_minimizers([s for _, s in masked])
    cap = u.default_capacity(len(mins))
    blob, size = t.model(tax, masked, cap)
    assert size == len(mins) == len(np.unique(u.fmix64_np(mins) >> np.uint64(35)))  # (no shared key: order free)
    m = t.write_case(tmp_path, c["lines"], records)
    st = build(m, tmp_path / "db", batch=997, mask_low_complexity=True)
    assert st["masked_bases"] == n_masked
    mc = dict(c, pairs=pairs, mins=mins, cap=cap, model=blob, size=size)
    assert_is_the_model(st, tmp_path / "db", mc)
    assert st["size"] < build(m, tmp_path / "plain", batch=997)["size"]


def assert_cells_equal(got, model_blob):
    (hdr, cells), (mhdr, mcells) = got, u.cells_of(model_blob)
    assert hdr == mhdr, (hdr, mhdr)
    bad = np.flatnonzero(cells != mcells)
    assert bad.size == 0, "cells %s: %s, the model has %s" % (bad[:8], cells[bad[:8]], mcells[bad[:8]])


def test_shared_keys_across_taxa(tmp_path):
    """two distinct minimizers with one compacted key, in different taxa: the second arrives at the first one's cell and the cell's
    value becomes the root.  One record a batch: the model's table of the file's order, cell for cell.  One batch: a valid table
    whose merged cells hold a leaf or the root, as the orders of the model allow"""
    cap = 1009
    lines, tax, dealt, mins = t.shared_key_case(cap)
    records = {x: [(n, s) for y, n, s in dealt if y == x] for x in (7, 8)}
    pairs = t.pairs_of(tax, records)  # all of taxon 7, then all of taxon 8: the order of the build
    blob, size = t.model(tax, pairs, cap)
    mhdr, mcells = u.cells_of(blob)
    counts = t.value_counts(mcells, 2, 4)
    assert size < len(mins) and counts[1] >= 1 and counts[2] > 0 and counts[3] > 0  # a merged cell holds the root
    m = t.write_case(tmp_path, lines, records)
    st = build(m, tmp_path / "seq", batch=64, capacity=cap)
    assert_cells_equal(table(tmp_path / "seq"), blob)
    assert st["size"] == size and [x["cells"] for x in st["taxon_stats"]] == counts[1:]
    # one batch, any order of arrival
    st = build(m, tmp_path / "one", capacity=cap)
    hdr, cells = table(tmp_path / "one")
    by_key = {}
    for x, s in pairs:
        (amb, mz), = u.lit.kmer_minimizers(u._shim(), s)
        by_key.setdefault(u.lit.fmix64(mz) >> bf.KEY_SHIFT, set()).add(tax.internal[x])
    for c in cells[cells != 0].tolist():
        owners = by_key[c >> 2]
        assert (c & 3) in (owners | {1} if len(owners) > 1 else owners), (hex(c), owners)
    bf.valid_table(hdr, np.where(cells != 0, (cells & ~np.uint32(3)) | np.uint32(2), 0).astype(np.uint32), mins, cap)
    assert sum(x["cells"] for x in st["taxon_stats"]) == st["size"] == hdr[1]


def test_wide(tmp_path):
    """300 leaves under the root: value_bits 9, a parent table beyond 256 entries, histogram bins beyond one wave's width"""
    c = t.wide_case()
    m = t.write_case(tmp_path, c["lines"], c["records"])
    st = build(m, tmp_path / "db")
    assert_is_the_model(st, tmp_path / "db", c)
    assert table(tmp_path / "db")[0][2:] == (23, 9) and st["taxon_stats"][0]["cells"] > 0


def test_one_taxon_by_manifest(tree, tmp_path):
    import nohuman_amd
    recs = tree["records"][t.A]
    fa = u.write_fasta(tmp_path / "x.fa", recs)
    m = t.write_manifest(tmp_path / "one.tsv", [(4242, 1, "one host", "x.fa")])
    st_m = build(m, tmp_path / "by_manifest")
    st_r = nohuman_amd.build_db([fa], str(tmp_path / "by_reference"), taxid=4242, taxon_name="one host")
    (hm, cm, om, tm), (hr, cr, orr, tr) = u.read_db(str(tmp_path / "by_manifest")), u.read_db(str(tmp_path / "by_reference"))
    assert om == orr and tm == tr and hm[2:] == (30, 2)
    u.same_table((hm, cm), (hr, cr))
    for k in ("sequences", "bases", "kmers", "ambiguous_kmers", "distinct_minimizers", "capacity", "size", "masked_bases", "taxa"):
        assert st_m[k] == st_r[k], k
    assert st_r["taxa"] == 2 and st_m["taxon_stats"] == st_r["taxon_stats"]
    assert st_r["taxon_stats"][1] == dict(taxid=4242, sequences=len(recs), bases=sum(len(s) for _, s in recs), kmers=st_r["kmers"],
                                          cells=st_r["size"])
    # the build of one taxon is the one it was: the model of tests/build_db_util.py
    seqs = [s for _, s in recs]
    blob, size = u.model_hash(seqs, st_r["capacity"], taxid=4242)
    u.same_table((hr, cr), u.cells_of(blob))
    assert t.parse_taxo(tr) == [(0, 0, 0, 0, "root"), (0, 2, 1, 1, "root"), (1, 0, 0, 4242, "one host")]


def _reads(tree):
    """150-base reads cut from what only A has, only B, A and B, all three, only C, and random ones -> [(id, sequence, taxid or
    None where the read is in no taxon)]"""
    rng = np.random.default_rng(77)
    st, rec = tree["stretches"], tree["records"]
    sources = (("a", rec[t.A][0][1], t.A), ("b", rec[t.B][0][1], t.B), ("ab", st["ab"], t.G), ("abc", st["abc"], 1),
               ("c", rec[t.C_][2][1], t.C_))
    reads = []
    for name, src, want in sources:
        src = src.upper()
        for i in range(6):
            while True:
                at = int(rng.integers(0, len(src) - 150))
                if b"N" not in src[at:at + 150]:
                    break
            reads.append((b"%s_%d" % (name.encode(), i), src[at:at + 150], want))
    reads += [(b"random_%d" % i, synth.random_seq(rng, 150), None) for i in range(6)]
    order = rng.permutation(len(reads))
    return [reads[i] for i in order]


def _report_counts(text):
    """a kraken2 report -> {taxid: (clade count, own count)}"""
    out = {}
    for ln in text.decode().splitlines():
        f = ln.split("\t")
        out[int(f[4])] = (int(f[1]), int(f[2]))
    return out


def test_end_to_end(tree, tmp_path):
    from nohuman_amd import engine
    from oracle import oracle as orc
    reads = _reads(tree)
    fq = tmp_path / "reads.fq"
    fq.write_bytes(b"".join(b"@" + n + b"\n" + s + b"\n+\n" + b"I" * len(s) + b"\n" for n, s, _ in reads))
    st = engine.run(str(tree["db"]), str(fq), str(tmp_path / "kept.fq"), calls=str(tmp_path / "calls.tsv"),
                    report=str(tmp_path / "report.txt"), kraken_output=str(tmp_path / "k.txt"))
    assert st.total_sequences == len(reads)
    rows = [ln.split(b"\t") for ln in (tmp_path / "calls.tsv").read_bytes().splitlines()]
    assert [r[1] for r in rows] == [n for n, _, _ in reads]
    for r, (n, _, want) in zip(rows, reads):
        assert (r[0], int(r[2])) == ((b"C", want) if want else (b"U", 0)), n
    # the oracle on the same three files
    odb = orc.OracleDB(directory=str(tree["db"]))
    odb.set(ambiguity_rule=u.rule())
    bases, offs = orc.pack_reads([s for _, s, _ in reads], False)
    exp, _ = odb.classify(bases, offs, False, 0.0)
    ext = [int(x) for x in odb.external_ids]
    assert ext == tree["tax"].external
    assert [(int(r[2]), int(r[4]), int(r[5]), int(r[6])) for r in rows] == \
        [(ext[int(e["call"])], int(e["total_kmers"]), int(e["clade_hits"]), int(e["hit_groups"])) for e in exp]
    krows = [ln.split(b"\t") for ln in (tmp_path / "k.txt").read_bytes().splitlines()]
    assert [int(r[2]) for r in krows] == [int(r[2]) for r in rows]
    # the report: every node, with the clade counts of the oracle's calls
    tax = tree["tax"]
    own = [0] * tax.node_count
    for e in exp:
        own[int(e["call"])] += 1
    clade = own[:]
    for i in range(tax.node_count - 1, 1, -1):
        clade[tax.parent[i]] += clade[i]
    report = (tmp_path / "report.txt").read_bytes()
    want = {tax.external[i]: (clade[i], own[i]) for i in range(1, tax.node_count)}
    want[0] = (own[0], own[0])
    assert _report_counts(report) == want and min(c for c, _ in want.values()) > 0
    assert want[1] == (30, 6) and want[t.G] == (18, 6)
    for name in ("root", "group G", "taxon A", "taxon B", "taxon C"):
        assert name.encode() in report
    kept = (tmp_path / "kept.fq").read_bytes()
    assert kept.count(b"\n") == 4 * 6 and kept.count(b"@random_") == 6


def test_cli(tree, tmp_path):
    d = tmp_path / "clidb"
    p = subprocess.run([BIN, "--build-db", str(d), "--taxa", tree["manifest"]], capture_output=True, timeout=300)
    err = p.stderr.decode(errors="replace")
    assert p.returncode == 0, err
    u.same_table(table(d), table(tree["db"]))
    assert u.read_db(str(d))[3] == u.read_db(str(tree["db"]))[3]
    for x, name in zip(tree["stats"]["taxon_stats"], ("root", "taxon C", "group G", "taxon A", "taxon B")):
        line = "%s (taxid %d): %d sequences, %d bases, %d cells" % (name, x["taxid"], x["sequences"], x["bases"], x["cells"])
        assert line in err, (line, err)
    reads = _reads(tree)
    fq = tmp_path / "reads.fq"
    fq.write_bytes(b"".join(b"@" + n + b"\n" + s + b"\n+\n" + b"I" * len(s) + b"\n" for n, s, _ in reads))
    p = subprocess.run([BIN, "--db", str(d), str(fq), "-o", str(tmp_path / "out.fq"), "--calls", str(tmp_path / "c.tsv"),
                        "-r", str(tmp_path / "r.txt")], capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode(errors="replace")
    rows = [ln.split(b"\t") for ln in (tmp_path / "c.tsv").read_bytes().splitlines()]
    assert [int(r[2]) for r in rows] == [want or 0 for _, _, want in reads]
    assert set(_report_counts((tmp_path / "r.txt").read_bytes())) == {0, 1, t.A, t.B, t.C_, t.G}


def test_without_a_manifest_nothing_changed(tree, tmp_path):
    """a build without taxa_file: the stats it had, and the two earlier layouts of the structs keep their sizes"""
    import ctypes as C
    from nohuman_amd import _lib
    recs = tree["records"][t.B]
    fa = u.write_fasta(tmp_path / "b.fa", recs)
    a = _lib.nh_build_args_v3()
    a.struct_size = 88  # the second layout: what lies behind it is not read, and 104 bytes of stats are written
    a.taxa_file = tree["manifest"].encode()
    paths = (C.c_char_p * 1)(os.fsencode(fa))
    a.n_fasta, a.fasta, a.out_dir = 1, paths, os.fsencode(str(tmp_path / "v2"))
    s = _lib.nh_build_stats_v3()
    C.memset(C.byref(s), 0xA5, C.sizeof(s))
    assert _lib.lib().nh_build_db(C.byref(a), C.byref(s)) == 0, _lib.lib().nh_last_error()
    assert bytes(s)[104:] == b"\xa5" * 8
    seqs = [q for _, q in recs]
    mins = u.fast_minimizers(seqs)
    assert (s.sequences, s.bases, s.distinct_minimizers, s.size, s.masked_bases) == (len(seqs), sum(map(len, seqs)), len(mins), len(mins), 0)
    hdr, cells, _, tb = u.read_db(str(tmp_path / "v2"))
    assert hdr[2:] == (30, 2) and t.parse_taxo(tb)[2][3:] == (9606, "Homo sapiens")
    blob, _ = u.model_hash(seqs, s.capacity)
    u.same_table((hdr, cells), u.cells_of(blob))
