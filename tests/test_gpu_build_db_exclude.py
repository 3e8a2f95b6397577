"""nh_build_db_exclude on the GPU (nohuman_amd/csrc/nh_build.hip: the EXCLUDE pass and INSERT with its filter) against
tests/exclude_model.py: a build that leaves out the host's minimizers that the sequences of an exclusion list carry too.

Tables are compared as tests/test_gpu_build_db.py compares them (header, occupied positions, sorted cells), which is the whole
table while no two KEPT minimizers share a compacted key: exclude_model.order_free asserts it on the CPU for every input so
compared.  Inputs that share a key on purpose are held to build_forge.valid_table on H \\ X."""
import os

import numpy as np
import pytest

from oracle import k2_literal as lit
from tests import build_db_util as u
from tests import build_forge as bf
from tests import exclude_model as xm
from tests import synth

pytestmark = pytest.mark.gpu
NH_EIO, NH_EDB, NH_ECAPACITY = -2, -3, -6
HOST_SEED, OTHER_SEED, DISJOINT_SEED = 1, 61, 62
# (record of B, start, length, reverse-complemented in A) -> planted into (record of A, at)
PLANTED = ((1, 300, 150, False, 2, 700), (4, 1200, 300, True, 5, 1500), (6, 2000, 220, False, 0, 40))
STAT_KEYS = ("sequences", "bases", "kmers", "ambiguous_kmers", "distinct_minimizers", "capacity", "size", "exclude_sequences",
             "exclude_bases", "exclude_kmers", "exclude_ambiguous_kmers", "excluded_minimizers", "kept_minimizers")


def build(paths, out_dir, batch=None, **kw):
    import nohuman_amd
    with pytest.MonkeyPatch.context() as mp:
        if batch is None:
            mp.delenv("NOHUMAN_BUILD_BATCH", raising=False)
        else:
            mp.setenv("NOHUMAN_BUILD_BATCH", str(batch))
        return nohuman_amd.build_db(paths, str(out_dir), **kw)


def table(d):
    hdr, cells, _, _ = u.read_db(str(d))
    return hdr, cells


def clean_of(s):
    return bytes(s).upper().replace(b"N", b"A")


def assert_model(st, d, m):
    """the stats and the table of a build against the model's"""
    assert st["distinct_minimizers"] == len(m["H"])
    assert st["excluded_minimizers"] == len(m["excluded"]) and st["kept_minimizers"] == len(m["kept"])
    assert st["capacity"] == m["capacity"] and st["size"] == m["size"]
    assert (st["kmers"], st["ambiguous_kmers"]) == (m["kmers"], m["ambiguous"])
    assert (st["exclude_sequences"], st["exclude_bases"], st["exclude_kmers"], st["exclude_ambiguous_kmers"]) == \
        (m["x_sequences"], m["x_bases"], m["x_kmers"], m["x_ambiguous"])
    # a look-up a run of equal minimizers, a run ending where a piece does: at least the model's runs, at most every clean k-mer
    assert m["x_lookups"] <= st["exclude_lookups"] <= m["x_kmers"] - m["x_ambiguous"]
    hdr, cells = table(d)
    u.same_table((hdr, cells), u.cells_of(m["table"]))
    assert hdr[1] == int((cells != 0).sum()) == m["size"]


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """host genome A with three stretches of the exclusion genome B (one reverse-complemented), the model (computed once) and the
    build with the list at small pieces"""
    tmp = tmp_path_factory.mktemp("exclude")
    a, b = u.genome(HOST_SEED), u.genome(OTHER_SEED)
    stretches = []
    for rb, start, n, rc, ra, at in PLANTED:
        s = clean_of(b[rb][1][start:start + n])
        b[rb] = (b[rb][0], b[rb][1][:start] + s + b[rb][1][start + n:])
        stretches.append(s)
        name, seq = a[ra]
        a[ra] = (name, seq[:at] + (synth.revcomp(s) if rc else s) + seq[at:])
    host, excl = [s for _, s in a], [s for _, s in b]
    m = xm.order_free(xm.model(host, excl))
    fa, fb = u.write_fasta(tmp / "a.fa", a), u.write_fasta(tmp / "b.fa", b)
    st = build([fa], tmp / "db", piece_kmers=300, exclude=[fb])
    return dict(tmp=tmp, a=a, b=b, host=host, excl=excl, m=m, fa=fa, fb=fb, db=tmp / "db", stats=st, stretches=stretches)


def test_planted_overlap(case):
    m = case["m"]
    assert 0 < len(m["excluded"]) < len(m["H"])
    for s in case["stretches"]:
        assert xm.brute_minimizers(s) <= m["excluded"]
    assert_model(case["stats"], case["db"], m)
    st = case["stats"]
    assert st["capacity"] == u.default_capacity(len(m["kept"])) < u.default_capacity(len(m["H"]))
    assert st["seconds_exclude"] > 0 and st["taxa"] == 2
    assert set(os.listdir(case["db"])) == set(u.DB_FILES)
    # whole sequences as pieces, and a single path instead of a list: the same
    st_w = build(case["fa"], case["tmp"] / "whole", exclude=case["fb"])
    assert [st_w[k] for k in STAT_KEYS] == [st[k] for k in STAT_KEYS]
    assert len(m["X"]) <= st_w["exclude_lookups"] <= st["exclude_lookups"]  # (a piece's first k-mer starts a run)
    u.same_table(table(case["tmp"] / "whole"), table(case["db"]))


def test_disjoint_exclusion_genome(case, tmp_path):
    other = u.genome(DISJOINT_SEED)
    assert not case["m"]["H"] & u.minimizers([s for _, s in other])[0]
    plain = build([case["fa"]], tmp_path / "plain", piece_kmers=300)
    st = build([case["fa"]], tmp_path / "db", piece_kmers=300, exclude=[u.write_fasta(tmp_path / "o.fa", other)])
    assert st["excluded_minimizers"] == 0 and st["kept_minimizers"] == st["distinct_minimizers"] == plain["distinct_minimizers"]
    assert (st["capacity"], st["size"]) == (plain["capacity"], plain["size"]) and "excluded_minimizers" not in plain
    u.same_table(table(tmp_path / "db"), table(tmp_path / "plain"))
    # an empty list is the plain build
    st = build([case["fa"]], tmp_path / "none", piece_kmers=300, exclude=[])
    assert "excluded_minimizers" not in st
    u.same_table(table(tmp_path / "none"), table(tmp_path / "plain"))


P_BORDER = 64


@pytest.fixture(scope="module")
def border_inputs():
    """a host of 73 chunks of 100 bases; an exclusion record that carries chunk j across the piece border 3 P (j + 1) of its own
    cut (pieces of P k-mers start every P bases), the chunk's middle at the offsets -36 .. +36 from the border; the same with an N
    at border + offset, inside the chunk; the models of both (exclude_model.model_fast: 30 kb in all)"""
    rng = np.random.default_rng(71)
    host = [synth.random_seq(rng, 100 * 73 + 50)]
    back = synth.random_seq(rng, 3 * P_BORDER * 75)
    plain, with_n = bytearray(back), bytearray(back)
    for j, off in enumerate(range(-36, 37)):
        border = 3 * P_BORDER * (j + 1)
        chunk = host[0][100 * j:100 * j + 100]
        for s in (plain, with_n):
            s[border + off - 50:border + off + 50] = chunk
        with_n[border + off] = ord("N")
    out = {}
    for name, s in (("plain", bytes(plain)), ("n", bytes(with_n))):
        recs = [(b"short", back[:34]), (b"carrier", s), (b"tail", back[-40:])]
        out[name] = (recs, xm.model_fast(host, [r for _, r in recs]))
    assert len(out["n"][1]["excluded"]) < len(out["plain"][1]["excluded"]) and out["n"][1]["x_ambiguous"] > 73 * 30
    return host, out


@pytest.mark.parametrize("batch", [None, 5000])
@pytest.mark.parametrize("form", ["plain", "n"])
def test_borders(border_inputs, tmp_path, form, batch):
    """the shared stretch across a piece border of the exclusion input at every offset, with and without an N there; with
    batches of 5000 bytes the 14 kb exclusion record is cut at batch ends as well"""
    host, forms = border_inputs
    recs, m = forms[form]
    if batch:
        cut = bf.batches_of([s for _, s in recs], batch)
        assert sum(1 for b in cut if any(i == 1 for i, _ in b)) >= 3  # (the carrier lies in three batches)
    fa = u.write_fasta(tmp_path / "h.fa", [(b"host", host[0])])
    fx = u.write_fasta(tmp_path / "x.fa", recs)
    st = build([fa], tmp_path / "db", batch=batch, piece_kmers=P_BORDER, exclude=[fx])
    assert_model(st, tmp_path / "db", m)


def test_order_and_duplication(case, tmp_path):
    """the exclusion records reversed, dealt to two files, and every record twice: the same stats and the same table -- each
    minimizer of the host is counted as excluded once, however often and in whatever order it is met"""
    b = case["b"]
    variants = {
        "reversed": [u.write_fasta(tmp_path / "r.fa", b[::-1])],
        "two_files": [u.write_fasta(tmp_path / "t2.fa", b[5:]), u.write_fasta(tmp_path / "t1.fa", b[:5])],
        "twice": [u.write_fasta(tmp_path / "d.fa", [r for r in b for _ in range(2)])],
    }
    want, ref = case["stats"], table(case["db"])
    same = [k for k in STAT_KEYS if not k.startswith("exclude_")]
    for name, paths in variants.items():
        st = build([case["fa"]], tmp_path / name, batch=7000 if name == "twice" else None, piece_kmers=300, exclude=paths)
        assert [st[k] for k in same] == [want[k] for k in same], name
        assert st["exclude_bases"] == (2 if name == "twice" else 1) * want["exclude_bases"]
        u.same_table(table(tmp_path / name), ref)


@pytest.fixture(scope="module")
def last_slot():
    """15 forged minimizers whose probe of the counting set starts at its last slot, at every size up to 262144 slots: ten for
    the host (they fill the last slot and, wrapping, the first nine), five of which the exclusion list carries too, and five for
    the exclusion list alone (their probes wrap, pass the ten and end at an empty slot)"""
    made = bf.forge(1, [(0, None)] * 15, np.random.default_rng(81), low_ones=18)
    assert all(lit.fmix64(m) & 0x3FFFF == 0x3FFFF for m, _ in made) and len({m for m, _ in made}) == 15
    return made


@pytest.mark.parametrize("random_bases,slots", [(20_000, 65536), (50_000, 131072), (100_000, 262144)])
def test_set_probe(last_slot, tmp_path, random_bases, slots):
    rng = np.random.default_rng(random_bases)
    fill = synth.random_seq(rng, random_bases)
    host = [(b"h%d" % i, r) for i, (_, r) in enumerate(last_slot[:10])] + [(b"fill", fill)]
    seqs = [s for _, s in host]
    assert bf.counting_set_slots(seqs, 128 << 20)[1] == [slots]  # (one batch: the set EXCLUDE probes has this many slots)
    both = [(b"b%d" % i, r) for i, (_, r) in enumerate(last_slot[5:10])]
    only = [(b"o%d" % i, r) for i, (_, r) in enumerate(last_slot[10:])]
    excl = only[:2] + both + only[2:] + [(b"other", synth.random_seq(rng, 3000))]
    mins = u.fast_minimizers(seqs)
    gone = np.array([m for m, _ in last_slot[5:10]], dtype=np.uint64)
    assert np.isin(gone, mins).all() and not np.isin(np.array([m for m, _ in last_slot[10:]], dtype=np.uint64), mins).any()
    assert not np.isin(u.fast_minimizers([s for _, s in excl]), np.setdiff1d(mins, gone)).any()
    kept = np.setdiff1d(mins, gone)
    cap = u.default_capacity(len(kept))
    u.assert_order_free_fast(kept, cap, apart=1024)
    fa, fx = u.write_fasta(tmp_path / "h.fa", host), u.write_fasta(tmp_path / "x.fa", excl)
    st = build([fa], tmp_path / "db", exclude=[fx])
    assert (st["distinct_minimizers"], st["excluded_minimizers"], st["kept_minimizers"]) == (len(mins), 5, len(kept))
    assert (st["capacity"], st["size"]) == (cap, len(kept))
    # the host without the five records, built without a list: the same table
    plain = build([u.write_fasta(tmp_path / "p.fa", host[:5] + host[10:])], tmp_path / "plain")
    assert (plain["distinct_minimizers"], plain["capacity"]) == (len(kept), cap)
    hdr, cells = table(tmp_path / "db")
    assert u.longest_run(cells) < 1024
    u.same_table((hdr, cells), table(tmp_path / "plain"))


def test_shared_compacted_key(tmp_path):
    """an excluded and a kept minimizer with one compacted key and one home: one exclusion is counted, the key's cell is there
    (for the kept one), and the table is a valid table of H \\ X"""
    cap = 1009
    rng = np.random.default_rng(91)
    (kept, r_kept), (gone, r_gone), (lone, r_lone) = bf.forge(cap, [(500, 0x2468ACE), (500, 0x2468ACE), (77, 0x1357)], rng)
    fill = [(b"f%d" % i, synth.random_seq(rng, 35)) for i in range(20)]
    host = [(b"kept", r_kept), (b"gone", r_gone), (b"lone", r_lone)] + fill
    m = xm.model([s for _, s in host], [r_gone, r_lone], capacity=cap)
    assert m["excluded"] == {gone, lone} and kept in m["kept"] and xm.shared_keys(m["kept"], m["excluded"]) == [gone]
    fa = u.write_fasta(tmp_path / "h.fa", host)
    fx = u.write_fasta(tmp_path / "x.fa", [(b"x1", r_gone), (b"x2", r_lone)])
    st = build([fa], tmp_path / "db", capacity=cap, exclude=[fx])
    assert (st["excluded_minimizers"], st["kept_minimizers"], st["distinct_minimizers"]) == (2, len(m["kept"]), len(m["H"]))
    hdr, cells = table(tmp_path / "db")
    bf.valid_table(hdr, cells, m["kept"], cap)
    assert st["size"] == hdr[1] == m["size"]
    assert cells[500] == 0x2468ACE << u.VALUE_BITS | 2 and cells[77] == 0
    assert xm.still_found(cells, m["excluded"], cap) == [gone]
    # only the one with the key excluded, the other way round: one exclusion either way, the cell stays
    st = build([fa], tmp_path / "db2", capacity=cap, exclude=[u.write_fasta(tmp_path / "x2.fa", [(b"x", r_kept)])])
    assert st["excluded_minimizers"] == 1 and table(tmp_path / "db2")[1][500] == 0x2468ACE << u.VALUE_BITS | 2


def test_everything_excluded(case, tmp_path):
    import nohuman_amd
    d = tmp_path / "db"
    copy = u.write_fasta(tmp_path / "copy_of_a.fa", case["a"][::-1], width=70)
    with pytest.raises(nohuman_amd.EngineError) as ei:
        build([case["fa"]], d, exclude=[copy])
    assert ei.value.code == NH_EDB and "every minimizer of the input is excluded" in ei.value.message
    assert not d.exists()
    # into a directory that holds a database: it stays, byte for byte
    build([case["fa"]], d)
    old = {n: (d / n).read_bytes() for n in u.DB_FILES}
    with pytest.raises(nohuman_amd.EngineError) as ei:
        build([case["fa"]], d, exclude=[copy], force=True)
    assert ei.value.code == NH_EDB
    assert set(os.listdir(d)) == set(u.DB_FILES) and {n: (d / n).read_bytes() for n in u.DB_FILES} == old
    # an exclusion file that is no FASTA: NH_EIO with its name, out_dir as it was; and the device builds on
    junk = tmp_path / "junk.fa"
    junk.write_bytes(b"this is no sequence file\nACGT\n")
    for d2, kw in ((tmp_path / "j", {}), (d, dict(force=True))):
        with pytest.raises(nohuman_amd.EngineError) as ei:
            build([case["fa"]], d2, exclude=[case["fb"], str(junk)], **kw)
        assert ei.value.code == NH_EIO and "junk.fa" in ei.value.message and "unrecognized file format" in ei.value.message
    assert not (tmp_path / "j").exists() and {n: (d / n).read_bytes() for n in u.DB_FILES} == old
    st = build([case["fa"]], tmp_path / "after", piece_kmers=300, exclude=[case["fb"]])
    assert st["excluded_minimizers"] == len(case["m"]["excluded"])
    u.same_table(table(tmp_path / "after"), table(case["db"]))


def test_given_capacity(case, tmp_path):
    import nohuman_amd
    m = case["m"]
    cap = 12007
    mc = xm.order_free(xm.model(case["host"], case["excl"], capacity=cap))
    st = build([case["fa"]], tmp_path / "db", capacity=cap, exclude=[case["fb"]])
    assert st["distinct_minimizers"] == len(m["H"]) > 0 and st["seconds_count"] > 0 and st["capacity"] == cap
    assert_model(st, tmp_path / "db", mc)
    bf.valid_table(*table(tmp_path / "db"), m["kept"], cap)
    # one cell more than the kept minimizers holds them (the excluded ones need none); exactly as many is a full table
    st = build([case["fa"]], tmp_path / "tight", capacity=len(m["kept"]) + 1, exclude=[case["fb"]])
    assert st["size"] == len(m["kept"]) < len(m["H"])
    with pytest.raises(nohuman_amd.EngineError) as ei:
        build([case["fa"]], tmp_path / "full", capacity=len(m["kept"]), exclude=[case["fb"]])
    assert ei.value.code == NH_ECAPACITY and "capacity" in ei.value.message and not (tmp_path / "full").exists()


@pytest.fixture(scope="module")
def manifest_inputs():
    """the tree of the taxa tests with a list that carries the stretch A and B share and a stretch of A alone, and the model's
    table of it (computed once)"""
    from oracle import minidb
    from tests import build_taxa_util as t
    c = t.tree_case()
    tax, st_ = c["tax"], c["stretches"]
    a_only = clean_of(c["records"][t.A][7][1][1000:1400])
    excl = [(b"ab", st_["ab"]), (b"a_only", a_only)]
    mins = lambda seq: xm._scan([seq])[0]  # noqa: E731
    X = xm._scan([s for _, s in excl])[0]
    H = set(c["mins"].tolist())
    kept = H - X
    assert mins(st_["ab"]) <= H & X and mins(a_only) <= H & X and not X & (mins(st_["ag"]) | mins(st_["abc"]))
    cap = u.default_capacity(len(kept))
    vb = minidb.value_bits_for(tax.node_count)
    blob, size = xm.build_hash_fast(tax, c["pairs"], X, cap)
    assert size == len(kept)
    return dict(c=c, excl=excl, mins=mins, X=X, H=H, kept=kept, cap=cap, vb=vb, blob=blob, size=size)


def manifest_build(tmp_path, mi, **kw):
    """the manifest build with the list against the model: the table as a set, the cells per node, the statistics"""
    from oracle import minidb
    from tests import build_taxa_util as t
    c, X, H, kept, cap, vb, blob, size, mins = (mi[k] for k in ("c", "X", "H", "kept", "cap", "vb", "blob", "size", "mins"))
    tax, st_ = c["tax"], c["stretches"]
    m = t.write_case(tmp_path, c["lines"], c["records"])
    st = build(None, tmp_path / "db", taxa=m, exclude=[u.write_fasta(tmp_path / "x.fa", mi["excl"])], **kw)
    assert (st["distinct_minimizers"], st["excluded_minimizers"], st["kept_minimizers"]) == (len(H), len(H & X), len(kept))
    assert (st["capacity"], st["size"], st["taxa"]) == (cap, size, tax.node_count - 1)
    hdr, cells = table(tmp_path / "db")
    u.same_table((hdr, cells), u.cells_of(blob))
    per = [0] + [n["cells"] for n in st["taxon_stats"]]
    assert per == t.value_counts(cells, vb, tax.node_count) and sum(per) == st["size"]
    db = lit.DB.from_images(minidb.opts_bytes(), tax.to_bytes(), (tmp_path / "db" / "hash.k2d").read_bytes())
    assert all(db.get(x) == 0 for x in H & X)
    assert {db.get(x) for x in mins(st_["ag"])} == {tax.internal[t.G]}
    assert {db.get(x) for x in mins(st_["abc"])} == {1}
    return st


def test_manifest_build(tmp_path, manifest_inputs):
    """the tree of the taxa tests with a list that carries the stretch A and B share and a stretch of A alone: both are stored
    under no taxon, the stretch A and G share stays at G, the one A, B and C share at the root"""
    manifest_build(tmp_path, manifest_inputs, piece_kmers=500)


def test_manifest_build_cut(tmp_path, manifest_inputs):
    """the same build (k_build_pieces<false, true, true>) with batches of 4096 bytes and pieces of 64 k-mers: records are cut at
    the batches' ends, a piece is shorter than a tile, and the result is the model's all the same"""
    seqs = [s for _, s in manifest_inputs["c"]["pairs"]]
    cut = bf.batches_of(seqs, 4096)
    assert len(cut) >= 16 and sum(1 for j in range(len(seqs)) if sum(any(i == j for i, _ in b) for b in cut) >= 2) >= 12
    st = manifest_build(tmp_path, manifest_inputs, batch=4096, piece_kmers=64)
    assert st["exclude_kmers"] == sum(len(s) - 34 for _, s in manifest_inputs["excl"])


def test_mask_low_complexity(tmp_path):
    """the host is masked, the exclusion input never: a microsatellite both carry is in H no more (masked), so it is neither kept
    nor counted as excluded; the unmasked stretch both carry is excluded"""
    from tests import dust_model as dm
    rng = np.random.default_rng(101)
    sat = dm.periodic(rng, 180, 3)
    shared = synth.random_seq(rng, 200)
    host = [synth.random_seq(rng, 900) + sat + synth.random_seq(rng, 700) + shared + synth.random_seq(rng, 500), synth.random_seq(rng, 1500)]
    excl = [synth.random_seq(rng, 400) + sat + synth.random_seq(rng, 300), shared + synth.random_seq(rng, 600)]
    assert dm.mask(host[0])[900:1080] == b"N" * 180
    m = xm.order_free(xm.model(host, excl, mask=True))
    unmasked = xm.model(host, excl)
    assert xm.brute_minimizers(shared) <= m["excluded"] < unmasked["excluded"] and len(m["H"]) < len(unmasked["H"])
    assert xm.brute_minimizers(sat) <= m["X"] and not xm.brute_minimizers(sat) & m["H"]
    fa = u.write_fasta(tmp_path / "h.fa", [(b"h%d" % i, s) for i, s in enumerate(host)])
    fx = u.write_fasta(tmp_path / "x.fa", [(b"x%d" % i, s) for i, s in enumerate(excl)])
    st = build([fa], tmp_path / "db", piece_kmers=200, mask_low_complexity=True, exclude=[fx])
    assert_model(st, tmp_path / "db", m)
    assert st["masked_bases"] == sum(dm.masked_count(s) for s in host) >= 180


def test_purpose_end_to_end(case, tmp_path):
    """reads from inside a planted stretch of B and from A alone, through the engine: the database built with the list leaves
    B's reads alone and still removes A's; the database built without it removes both"""
    from nohuman_amd import engine
    rng = np.random.default_rng(111)
    reads = []
    for i in range(30):
        s = case["stretches"][i % 3]
        p = int(rng.integers(0, len(s) - 100 + 1))
        r = s[p:p + 100]
        reads.append((b"b%d" % i, synth.revcomp(r) if i % 2 else r, "b"))
    a0 = u.genome(HOST_SEED)
    whole = b"\n".join(case["host"]).upper()
    while len(reads) < 60:
        s = a0[int(rng.integers(0, len(a0)))][1]
        p = int(rng.integers(0, len(s) - 100))
        r = s[p:p + 100].upper()
        if b"N" not in r and r in whole:  # (a stretch of A that no planting cut)
            reads.append((b"a%d" % len(reads), r, "a"))
    fq = tmp_path / "reads.fq"
    fq.write_bytes(b"".join(b"@" + n + b"\n" + s + b"\n+\n" + b"I" * len(s) + b"\n" for n, s, _ in reads))
    plain = tmp_path / "plain"
    build([case["fa"]], plain)
    calls = {}
    for name, d in (("with", case["db"]), ("without", plain)):
        o = tmp_path / ("out_" + name)
        o.mkdir()
        st = engine.run(str(d), str(fq), str(o / "kept.fq"), calls=str(o / "calls.tsv"), threads=2)
        assert st.total_sequences == len(reads)
        rows = [ln.split(b"\t") for ln in (o / "calls.tsv").read_bytes().splitlines()]
        assert [r[1] for r in rows] == [n for n, _, _ in reads]
        calls[name] = {r[1]: r[0] for r in rows}
        kept = (o / "kept.fq").read_bytes()
        assert kept.count(b"\n") == 4 * sum(1 for v in calls[name].values() if v == b"U")
    for n, _, src in reads:
        assert calls["without"][n] == b"C", n
        assert calls["with"][n] == (b"U" if src == "b" else b"C"), n


def test_input_formats(case, tmp_path):
    """the exclusion list as gzip, with CRLF, wrapped at 60 columns and as FASTQ: the stats of the plain file"""
    b = case["b"]
    fq = tmp_path / "b.fq"
    fq.write_bytes(b"".join(b"@" + n + b"\n" + s + b"\n+\n" + b"I" * len(s) + b"\n" for n, s in b))
    forms = {
        "gzip": u.write_fasta(tmp_path / "b.fa.gz", b, gz=True),
        "crlf": u.write_fasta(tmp_path / "c.fa", b, crlf=True),
        "unwrapped": u.write_fasta(tmp_path / "u.fa", b, width=0),  # (the fixture's file is wrapped at 60 columns)
        "fastq": str(fq),
    }
    want = case["stats"]
    assert b"\n" in open(case["fb"], "rb").read(200)[30:] and all(len(s) > 60 for _, s in b)
    for name, path in forms.items():
        st = build([case["fa"]], tmp_path / name, piece_kmers=300, threads=2, exclude=[path])
        assert [st[k] for k in STAT_KEYS] == [want[k] for k in STAT_KEYS], name
        u.same_table(table(tmp_path / name), table(case["db"]))
