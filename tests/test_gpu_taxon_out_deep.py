"""Per-taxon outputs beyond the toy tree: a database made by the project's own builder on caterpillar(60) (tests/taxo_forge.py),
selectors nested four deep, eight selectors (NH_MAX_TAXON_OUTS), two batches; and the same database end to end.  The cases run
through test_gpu_taxon_out.Case with the database's directory and the tree's parent map; tests/test_taxo_forge.py asserts on
the CPU where the reads are called and which selector takes them."""
import pytest

from oracle import oracle as orc
from tests import build_db_util as u
from tests import build_taxa_util as t
from tests import taxo_forge as tf
from tests import taxout_model as tm
from tests.test_gpu_build_db_taxa import _report_counts, assert_is_the_model, build
from tests.test_gpu_taxon_out import Case, bins_end

pytestmark = pytest.mark.gpu
ENV = {"NOHUMAN_BATCH_FRAGS": "1000"}  # two batches


def _fastq(reads):
    return b"".join(b"@%s\n%s\n+\n%s\n" % (n, s, b"I" * len(s)) for n, s in reads)


@pytest.fixture(scope="module")
def deep(tmp_path_factory):
    """the caterpillar(60) database, built once and held to its model before it is used; the reads as FASTQ files"""
    tmp = tmp_path_factory.mktemp("deep")
    c = tf.deep_case()
    st = build(t.write_case(tmp, c["lines"], c["records"]), tmp / "db")
    assert_is_the_model(st, tmp / "db", c)
    tf.assert_cells_are_the_lcas(u.read_db(str(tmp / "db"))[1], c)
    reads = tf.deep_reads()
    (tmp / "r1.fq").write_bytes(_fastq([(n, r) for n, r, _, _ in reads]))
    (tmp / "r2.fq").write_bytes(_fastq([(n, m) for n, _, m, _ in reads]))
    return dict(c, tmp=tmp, db=str(tmp / "db"), reads=reads, in1=str(tmp / "r1.fq"), in2=str(tmp / "r2.fq"),
                edges=tf.edges_of(c["parent"]))


def _fetched(c, sel, batch=1000):
    """what a run with a host codec fetches of the bins' buffers: per batch and mate as far as the last bin reaches, the bins laid
    out as bins_end says.  Every read of the pool is classified, so the keep_human output holds the batches' records in order"""
    total = 0
    for mi in range(len(c.mates)):
        recs = tm.records(c.keep[mi], True)
        for at in range(0, len(recs), batch):
            files, _ = tm.partition(b"".join(recs[at:at + batch]), True, c.parent, sel)
            total += bins_end([len(f) for f in files])
    return total


def _calls(deep, tmp, paired):
    """the external taxid of every read's call, through the calls table"""
    from nohuman_amd import engine
    engine.run(deep["db"], deep["in1"], str(tmp / "o1.fq"), in2=deep["in2"] if paired else None, out2=str(tmp / "o2.fq") if paired else None,
               calls=str(tmp / "calls.tsv"), threads=4)
    rows = [ln.split(b"\t") for ln in (tmp / "calls.tsv").read_bytes().splitlines()]
    assert [r[1] for r in rows] == [n for n, _, _, _ in deep["reads"]]
    return [int(r[2]) for r in rows]


@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_deep_database_eight_selectors(deep, tmp_path, paired):
    calls = _calls(deep, tmp_path, paired)
    assert calls == [w for _, _, _, w in deep["reads"]]
    c = Case(tmp_path, "deep", deep["in1"], deep["in2"] if paired else None, env=ENV, db=deep["db"], parent=deep["edges"])
    assert c.ref.total_sequences == len(calls) > 1000 and c.ref.classified == len(calls)
    # four nested levels and the largest number of selectors
    counts, trace = c.check(tf.DEEP_SEL_NESTED)
    assert counts == [len(g) for g in tm.route_calls(calls, deep["edges"], tf.DEEP_SEL_NESTED)]
    assert trace[2] == _fetched(c, tf.DEEP_SEL_NESTED)
    assert counts[6] == 0 and all(n for i, n in enumerate(counts) if i != 6) and sum(counts) == len(calls)
    at12 = {n for (n, _, _, _), w in zip(deep["reads"], calls) if w == tf.C(12)}
    in10 = {rec.split(b"\n", 1)[0][1:].split(b" ")[0] for rec in tm.records((tmp_path / "deep_s1" / "t1_1.fq").read_bytes(), True)}
    assert at12 and at12 <= in10  # a read called at C_12 lands in C_10's file
    # eight taxids, no "other"
    counts, trace = c.check(tf.DEEP_SEL_EIGHT)
    assert all(counts) and sum(counts) < len(calls) and trace[2] == _fetched(c, tf.DEEP_SEL_EIGHT)
    assert counts == [len(g) for g in tm.route_calls(calls, deep["edges"], tf.DEEP_SEL_EIGHT)]
    # the bottom of the chain alone
    counts, _ = c.check(tf.DEEP_SEL_BOTTOM)
    assert counts == [sum(1 for w in calls if w in (tf.C(60), tf.L(60)))] and counts[0] > 0


def test_deep_database_gzip(deep, tmp_path):
    c = Case(tmp_path, "deepgz", deep["in1"], None, codec=2, env=ENV, db=deep["db"], parent=deep["edges"])
    counts, trace = c.check(tf.DEEP_SEL_NESTED)
    assert counts[6] == 0 and sum(counts) == len(deep["reads"]) and trace[2] == 0


def test_end_to_end_on_the_deep_database(deep, tmp_path):
    """calls, the oracle on the built directory and the report's clade counts, in the manner of
    test_gpu_build_db_taxa.test_end_to_end"""
    from nohuman_amd import engine
    reads, tax = deep["reads"], deep["tax"]
    anc = tf.ancestor_sets(deep["parent"])
    st = engine.run(deep["db"], deep["in1"], str(tmp_path / "kept.fq"), calls=str(tmp_path / "calls.tsv"), report=str(tmp_path / "report.txt"),
                    kraken_output=str(tmp_path / "k.txt"))
    assert st.total_sequences == st.classified == len(reads)
    rows = [ln.split(b"\t") for ln in (tmp_path / "calls.tsv").read_bytes().splitlines()]
    assert [r[1] for r in rows] == [n for n, _, _, _ in reads]
    # lca_by_sets of the taxa each read was cut from
    for r, (n, s, _, _) in zip(rows, reads):
        assert (r[0], int(r[2])) == (b"C", tf.lca_by_sets(deep["parent"], tf.holders(deep, s), anc)), n
    # the oracle on the same three files
    odb = orc.OracleDB(directory=deep["db"])
    odb.set(ambiguity_rule=u.rule())
    exp, _ = odb.classify(*orc.pack_reads([s for _, s, _, _ in reads], False), False, 0.0)
    ext = [int(x) for x in odb.external_ids]
    assert ext == tax.external
    assert [(int(r[2]), int(r[4]), int(r[5]), int(r[6])) for r in rows] == \
        [(ext[int(e["call"])], int(e["total_kmers"]), int(e["clade_hits"]), int(e["hit_groups"])) for e in exp]
    krows = [ln.split(b"\t") for ln in (tmp_path / "k.txt").read_bytes().splitlines()]
    assert [int(r[2]) for r in krows] == [int(r[2]) for r in rows]
    # the report: the oracle's calls summed up the tree
    own = [0] * tax.node_count
    for e in exp:
        own[int(e["call"])] += 1
    clade = own[:]
    for i in range(tax.node_count - 1, 1, -1):
        clade[tax.parent[i]] += clade[i]
    got = _report_counts((tmp_path / "report.txt").read_bytes())
    want = {tax.external[i]: (clade[i], own[i]) for i in range(1, tax.node_count) if clade[i]}
    assert {k: v for k, v in got.items() if v[0]} == want
    assert want[1] == (len(reads), 0) and want[tf.C(1)][0] == len(reads) and want[tf.C(60)] == (32, 16)
    assert (tmp_path / "kept.fq").read_bytes() == b""
