"""nh_extend_db on the GPU: taxa added to an existing database without the sequences it was made from.  The extended directory is
held to a build of the union in one go at the base's capacity (build_db_util.same_table on hash.k2d, opts.k2d and taxo.k2d byte
for byte) and to the numpy model (tests/extend_model.py), which starts from the base's own files.  The base is built at a load
of 0.4 unless a test says otherwise, and its three files are hashed before and after every extension."""
import contextlib
import hashlib
import os
import subprocess

import numpy as np
import pytest

from oracle import minidb
from tests import build_db_util as u
from tests import build_taxa_util as t
from tests import dust_model as dm
from tests import extend_cases as xc
from tests import extend_model as xm
from tests import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "nohuman_amd", "bin", "nohuman")
ECAPACITY = -6


@contextlib.contextmanager
def _env(batch):
    with pytest.MonkeyPatch.context() as mp:
        if batch is None:
            mp.delenv("NOHUMAN_BUILD_BATCH", raising=False)
        else:
            mp.setenv("NOHUMAN_BUILD_BATCH", str(batch))
        yield


def build(out_dir, taxa=None, fasta=None, batch=None, **kw):
    import nohuman_amd
    with _env(batch):
        return nohuman_amd.build_db(fasta, str(out_dir), taxa=taxa, **kw)


def extend(base, out_dir, fasta=None, batch=None, **kw):
    import nohuman_amd
    with _env(batch):
        return nohuman_amd.extend_db(str(base), str(out_dir), fasta, **kw)


def digest(d):
    return {f: hashlib.sha256(open(os.path.join(str(d), f), "rb").read()).hexdigest() for f in sorted(os.listdir(str(d)))}


def table(d):
    hdr, cells, _, _ = u.read_db(str(d))
    return hdr, cells


def base_files(d):
    with open(os.path.join(str(d), "hash.k2d"), "rb") as f:
        hb = f.read()
    with open(os.path.join(str(d), "taxo.k2d"), "rb") as f:
        tb = f.read()
    return hb, tb


def make_base(tmp, c, **kw):
    """the case's base by the GPU builder at BASE_LOAD (a base of one taxon: the build without a manifest)"""
    d = tmp / "base"
    if len(c["base_lines"]) == 1:
        (taxid, _, name), = c["base_lines"]
        fa = u.write_fasta(tmp / "base.fa", c["base_records"][taxid])
        st = build(d, fasta=[fa], taxid=taxid, taxon_name=name, load_factor=xc.BASE_LOAD, **kw)
    else:
        os.makedirs(tmp / "b", exist_ok=True)
        st = build(d, taxa=t.write_case(tmp / "b", c["base_lines"], c["base_records"]), load_factor=xc.BASE_LOAD, **kw)
    assert st["capacity"] == c["cap"]
    return d, st


def one_shot(tmp, c, **kw):
    os.makedirs(tmp / "u", exist_ok=True)
    d = tmp / "oneshot"
    st = build(d, taxa=t.write_case(tmp / "u", c["union_lines"], c["union_records"]), capacity=c["cap"], **kw)
    return d, st


def add_manifest(tmp, c):
    os.makedirs(tmp / "a", exist_ok=True)
    return t.write_case(tmp / "a", c["add_lines"], c["add_records"], name="add.tsv")


def assert_extended(st, out, base, base_st, c, shot, model):
    """the extended directory and the stats of the call against the build in one go and the model"""
    tax = c["union_tax"]
    vb = max(model["old_vb"], minidb.value_bits_for(tax.node_count))
    hdr, cells, ob, tb = u.read_db(str(out))
    shdr, scells, sob, stb = u.read_db(str(shot))
    assert hdr == shdr == (c["cap"], model["size"], 32 - vb, vb)
    u.same_table((hdr, cells), (shdr, scells))
    u.same_table((hdr, cells), u.cells_of(model["hash"]))
    assert ob == sob == u.read_db(str(base))[2] and tb == stb
    assert st["shadowed_cells"] == model["shadowed"] == 0
    bhdr = table(base)[0]
    assert (st["base_size"], st["base_nodes"], st["base_value_bits"]) == (bhdr[1], c["base_tax"].node_count, bhdr[3])
    assert st["nodes_added"] == tax.node_count - c["base_tax"].node_count
    assert (st["capacity"], st["size"], st["taxa"]) == (c["cap"], model["size"], tax.node_count - 1)
    assert st["cells_added"] == model["cells_added"] == st["size"] - st["base_size"] and st["load"] == st["size"] / st["capacity"]
    ts = st["taxon_stats"]
    assert [x["taxid"] for x in ts] == tax.external[1:]
    assert [x["cells"] for x in ts] == model["cells"][1:] == t.value_counts(scells, vb, tax.node_count)[1:]
    assert [x["base_cells"] for x in ts] == model["base_cells"][1:] and sum(x["base_cells"] for x in ts) == st["base_size"]
    assert [(x["sequences"], x["bases"], x["kmers"]) for x in ts] == t.per_taxon(c["add_pairs"], tax)[1:]
    seqs = [s for _, s in c["add_pairs"]]
    assert (st["sequences"], st["bases"]) == (len(seqs), sum(map(len, seqs)))


def run_case(tmp, name, capfd=None, batch=None, **kw):
    c = xc.case(name)
    base, base_st = make_base(tmp, c)
    before = digest(base)
    out = tmp / "extended"
    if capfd is not None:
        capfd.readouterr()
    if name == "one":  # one taxon without a manifest
        (taxid, _, tname), = c["add_lines"]
        st = extend(base, out, [u.write_fasta(tmp / "add.fa", c["add_records"][taxid])], taxid=taxid, taxon_name=tname, batch=batch, **kw)
    else:
        st = extend(base, out, taxa=add_manifest(tmp, c), batch=batch, **kw)
    trace = capfd.readouterr().err if capfd is not None else ""
    assert digest(base) == before
    shot, _ = one_shot(tmp, c)
    model = xm.extend(*base_files(base), c["add_lines"], c["add_pairs"])
    assert_extended(st, out, base, base_st, c, shot, model)
    return c, st, model, trace


@pytest.mark.parametrize("name,old_vb,new_vb,rewritten", [("one", 2, 2, False), ("two", 2, 3, True), ("tree_wide", 3, 9, True), ("between", 2, 3, True)])
def test_extension_is_the_build_in_one_go(tmp_path, capfd, monkeypatch, name, old_vb, new_vb, rewritten):
    monkeypatch.setenv("NOHUMAN_TRACE", "1")
    c, st, model, trace = run_case(tmp_path, name, capfd)
    assert (model["old_vb"], model["new_vb"]) == (old_vb, new_vb) == (st["base_value_bits"], table(tmp_path / "extended")[0][3])
    assert ("table rewritten" if rewritten else "table as it was") in trace, trace  # (a) needs no re-key pass
    if name == "between":
        assert model["remap"] == [0, 1, 2, 4] and st["taxon_stats"][3]["sequences"] == 1 and st["taxon_stats"][3]["base_cells"] > 0
    if name == "tree_wide":
        assert model["remap"] == [0, 1, 2, 3, 304, 305]  # the 300 leaves are children of the root: A and B come behind them
    if name == "one":
        assert model["remap"] == [0, 1, 2] and st["nodes_added"] == 1


def test_batch_and_piece_borders(tmp_path):
    run_case(tmp_path, "two", batch=4096, piece_kmers=64)


@pytest.mark.parametrize("cap", [300001, 300002, 300003])
def test_the_vector_tail(tmp_path, cap):
    """a table whose last uint4 holds one, two or three cells: every cell of the base against the model, cell for cell"""
    assert cap % 4 in (1, 2, 3)
    big = u.genome(631, n_seq=8, length=25000)
    base = tmp_path / "base"
    bst = build(base, fasta=[u.write_fasta(tmp_path / "big.fa", big)], taxid=10, taxon_name="ten", capacity=cap)
    before = digest(base)
    lines = [(20, 1, "twenty"), (30, 1, "thirty")]
    records = {20: u.genome(632, n_seq=1), 30: u.genome(633, n_seq=1)}
    tax = t.taxonomy_of([(10, 1, "ten")] + lines)
    st = extend(base, tmp_path / "out", taxa=t.write_case(tmp_path, lines, records, name="add.tsv"))
    assert digest(base) == before
    model = xm.extend(*base_files(base), lines, t.pairs_of(tax, records))
    assert (model["old_vb"], model["new_vb"]) == (2, 3)
    hdr, cells = table(tmp_path / "out")
    mhdr, mcells = u.cells_of(model["hash"])
    assert hdr == mhdr == (cap, bst["size"] + st["cells_added"], 29, 3) and st["shadowed_cells"] == model["shadowed"]
    u.same_table((hdr, cells), (mhdr, mcells))
    was = table(base)[1] != 0  # a cell of the base never moves, and its key and value do not depend on the order of arrival
    assert np.array_equal(cells[was], mcells[was]) and was.sum() == bst["size"] > 60000
    assert [x["base_cells"] for x in st["taxon_stats"]] == model["base_cells"][1:] == [0, bst["size"], 0, 0]


def test_shadowed_cells(tmp_path):
    import nohuman_amd
    from oracle import oracle as orc
    s = xc.shadow_case()
    cap, K, tax = s["cap"], s["K"], s["tax"]
    base = tmp_path / "base"
    bst = build(base, taxa=t.write_case(tmp_path, s["lines"], s["records"], width=0), capacity=cap, batch=64)  # (a record a batch: in file order)
    bcells = table(base)[1]
    assert bst["size"] == 8 and bcells[cap - 1] == (2 * K) << 2 | tax.internal[xc.X_ID] and bcells[0] == (2 * K + 1) << 2 | tax.internal[xc.Y_ID]
    before = digest(base)
    zm, zr = s["z_filler"]
    os.makedirs(tmp_path / "z")
    z = t.write_case(tmp_path / "z", [s["z_line"]], {xc.Z_ID: [(b"zf", zr)]}, name="z.tsv", width=0)
    st = extend(base, tmp_path / "out", taxa=z)
    model = xm.extend(*base_files(base), [s["z_line"]], forged=[(xc.Z_ID, zm)])
    hdr, cells = table(tmp_path / "out")
    assert hdr == (cap, 9, 29, 3) and st["shadowed_cells"] == model["shadowed"] == 1 and st["cells_added"] == 1
    assert cells[cap - 1] == cells[0] == K << 3 | 1  # both cells: the key K, the root
    assert np.array_equal(cells, u.cells_of(model["hash"])[1])  # (no two additions: nothing depends on the order of arrival)
    assert [x["base_cells"] for x in st["taxon_stats"]] == [2, 3, 3, 0] and [x["cells"] for x in st["taxon_stats"]] == [2, 3, 3, 1]
    # a read that carries m2 meets the root, in cell 0 or in cell capacity - 1; so does one with m1; a filler of Y is Y's
    reads = [s["r2"], s["records"][xc.Y_ID][1][1], s["records"][xc.X_ID][0][1]]
    bases, offs = orc.pack_reads(reads, False)
    odb = orc.OracleDB(directory=str(tmp_path / "out"))
    odb.set(ambiguity_rule=u.rule(), minimum_hit_groups=1)
    exp, _ = odb.classify(bases, offs, False, 0.0)
    with nohuman_amd.Engine.open(str(tmp_path / "out")) as e:
        e.set_options(minimum_hit_groups=1)
        got = e.classify(bases, offs)
    assert got["call"].tolist() == exp["call"].tolist() == [1, model["tax"].internal[xc.Y_ID], 1]
    # Z with a third minimizer of the key K and the same home: the first cell stays the root, no cell is claimed for it
    os.makedirs(tmp_path / "z4")
    z4 = t.write_case(tmp_path / "z4", [s["z_line"]], {xc.Z_ID: [(b"zf", zr), (b"m4", s["r4"])]}, name="z.tsv", width=0)
    st4 = extend(base, tmp_path / "out4", taxa=z4)
    assert st4["cells_added"] == 1 and st4["shadowed_cells"] == 1 and np.array_equal(table(tmp_path / "out4")[1], cells)
    assert digest(base) == before


def test_capacity(tmp_path):
    import nohuman_amd
    host = u.genome(641)
    fa = u.write_fasta(tmp_path / "host.fa", host)
    distinct = len(u.fast_minimizers([s for _, s in host]))
    # a base with eight free cells
    tight = tmp_path / "tight"
    bst = build(tight, fasta=[fa], taxid=10, taxon_name="ten", capacity=distinct + 8)
    assert bst["size"] == distinct
    before = digest(tight)
    more = u.write_fasta(tmp_path / "more.fa", u.genome(642, n_seq=4))
    with pytest.raises(nohuman_amd.EngineError) as ei:
        extend(tight, tmp_path / "out", [more], taxid=30, taxon_name="thirty")
    assert ei.value.code == ECAPACITY and "8 free cells" in str(ei.value) and not (tmp_path / "out").exists() and digest(tight) == before
    # a ceiling of 0.5 on a base at 0.4: a quarter of the base's minimizers more cross it, a sixteenth do not
    base = tmp_path / "base"
    bst = build(base, fasta=[fa], taxid=10, taxon_name="ten", load_factor=0.4)
    before = digest(base)
    assert abs(bst["size"] / bst["capacity"] - 0.4) < 1e-3
    with pytest.raises(nohuman_amd.EngineError) as ei:
        extend(base, tmp_path / "out", [more], taxid=30, taxon_name="thirty", max_load=0.5)
    assert ei.value.code == ECAPACITY and "ceiling" in str(ei.value) and not (tmp_path / "out").exists() and digest(base) == before
    less = u.write_fasta(tmp_path / "less.fa", u.genome(642, n_seq=1)[:1])
    st = extend(base, tmp_path / "under", [less], taxid=30, taxon_name="thirty", max_load=0.5)
    assert 0.4 < st["load"] < 0.5 and digest(base) == before
    assert extend(base, tmp_path / "default_ceiling", [more], taxid=30, taxon_name="thirty")["load"] > 0.5


def test_with_mask_low_complexity(tmp_path):
    """the masked extension of a masked base is the masked build in one go"""
    c = dict(xc.case("two"))
    rng = np.random.default_rng(651)
    add = {k: list(v) for k, v in c["add_records"].items()}
    for taxid, i, at, s in ((20, 0, 300, dm.periodic(rng, 120, 2)), (30, 1, 1000, b"A" * 60), (30, 2, 50, b"CAG" * 30)):
        n, seq = add[taxid][i]
        add[taxid][i] = (n, seq[:at] + s + seq[at + len(s):])
    union = {**c["union_records"], **add}
    c.update(add_records=add, union_records=union, add_pairs=t.pairs_of(c["union_tax"], add), union_pairs=t.pairs_of(c["union_tax"], union))
    n_masked = sum(dm.masked_count(s) for _, s in c["add_pairs"])
    assert n_masked > 150
    base = tmp_path / "base"
    (taxid, _, name), = c["base_lines"]
    bst = build(base, fasta=[u.write_fasta(tmp_path / "base.fa", c["base_records"][taxid])], taxid=taxid, taxon_name=name,
                load_factor=xc.BASE_LOAD, mask_low_complexity=True)
    c["cap"] = bst["capacity"]
    before = digest(base)
    st = extend(base, tmp_path / "out", taxa=add_manifest(tmp_path, c), mask_low_complexity=True)
    assert st["masked_bases"] == n_masked and digest(base) == before
    shot, sst = one_shot(tmp_path, c, mask_low_complexity=True)
    assert sst["size"] == st["size"]
    u.same_table(table(tmp_path / "out"), table(shot))
    assert u.read_db(str(tmp_path / "out"))[2:] == u.read_db(str(shot))[2:]
    model = xm.extend(*base_files(base), c["add_lines"], [(x, dm.mask(s)) for x, s in c["add_pairs"]])
    u.same_table(table(tmp_path / "out"), u.cells_of(model["hash"]))
    assert extend(base, tmp_path / "plain", taxa=add_manifest(tmp_path, c))["size"] > st["size"]


HOST, DECOY = 10, 30


@pytest.fixture(scope="module")
def decoy(tmp_path_factory):
    """a host genome as the base, a decoy that shares a 3 kb stretch with it as the addition (one taxon, without a manifest)"""
    tmp = tmp_path_factory.mktemp("extend_decoy")
    rng = np.random.default_rng(661)
    shared = synth.random_seq(rng, 3000)
    host, dec = u.genome(662), u.genome(663, n_seq=4)
    host[2] = (host[2][0], host[2][1][:500] + shared + host[2][1][500:])
    dec[1] = (dec[1][0], dec[1][1][:900] + shared + dec[1][1][900:])
    lines = [(HOST, 1, "the host"), (DECOY, 1, "the decoy")]
    c = xc._case(lines[:1], {HOST: host}, lines[1:], {DECOY: dec})
    base, bst = make_base(tmp, c)
    before = digest(base)
    fa = u.write_fasta(tmp / "decoy.fa", dec)
    st = extend(base, tmp / "extended", [fa], taxid=DECOY, taxon_name="the decoy")
    assert digest(base) == before
    shot, _ = one_shot(tmp, c)
    model = xm.extend(*base_files(base), c["add_lines"], c["add_pairs"])
    assert_extended(st, tmp / "extended", base, bst, c, shot, model)
    return dict(c, tmp=tmp, base=base, out=tmp / "extended", shot=shot, stats=st, shared=shared, host=host, decoy=dec, fa=fa, before=before)


def test_end_to_end(decoy, tmp_path):
    rng = np.random.default_rng(664)
    sources = (("host", decoy["host"][0][1], False), ("decoy", decoy["decoy"][0][1], True), ("shared", decoy["shared"], True))
    reads = []
    for name, src, _ in sources:
        src = src.upper()
        for i in range(8):
            while True:
                at = int(rng.integers(0, len(src) - 150))
                if b"N" not in src[at:at + 150]:
                    break
            reads.append((b"%s_%d" % (name.encode(), i), src[at:at + 150]))
    reads += [(b"random_%d" % i, synth.random_seq(rng, 150)) for i in range(8)]
    reads = [reads[i] for i in rng.permutation(len(reads))]
    fq = tmp_path / "reads.fq"
    fq.write_bytes(b"".join(b"@" + n + b"\n" + s + b"\n+\n" + b"I" * len(s) + b"\n" for n, s in reads))
    outs = {}
    for which in ("out", "shot"):
        o = tmp_path / which
        o.mkdir()
        p = subprocess.run([BIN, "--db", str(decoy[which]), "--host-taxid", str(HOST), str(fq), "-o", str(o / "kept.fq"), "-k", str(o / "k.txt"),
                            "--calls", str(o / "calls.tsv")], capture_output=True, timeout=300)
        assert p.returncode == 0, p.stderr.decode(errors="replace")
        outs[which] = {f: (o / f).read_bytes() for f in ("kept.fq", "k.txt", "calls.tsv")}
    assert outs["out"] == outs["shot"]
    rows = {r[1]: (r[0], int(r[2])) for r in (ln.split(b"\t") for ln in outs["out"]["calls.tsv"].splitlines())}
    kept = outs["out"]["kept.fq"]
    for n, _ in reads:
        kind = n.split(b"_")[0]
        assert rows[n] == {b"host": (b"C", HOST), b"decoy": (b"C", DECOY), b"shared": (b"C", 1), b"random": (b"U", 0)}[kind], n
        assert (b"@" + n + b"\n" in kept) == (kind != b"host"), n  # the reads of the shared stretch are kept


def test_cli(decoy, tmp_path):
    m = t.write_manifest(tmp_path / "add.tsv", [(DECOY, 1, "the decoy", decoy["fa"])])
    d = tmp_path / "clidb"
    p = subprocess.run([BIN, "--build-db", str(d), "--extend-db", str(decoy["base"]), "--taxa", m, "-v"], capture_output=True, timeout=300)
    err = p.stderr.decode(errors="replace")
    assert p.returncode == 0, err
    assert digest(decoy["base"]) == decoy["before"]
    u.same_table(table(d), table(decoy["out"]))
    assert u.read_db(str(d))[2:] == u.read_db(str(decoy["out"]))[2:]
    st = decoy["stats"]
    assert "%d nodes added" % st["nodes_added"] in err and "%d cells added" % st["cells_added"] in err and "%d shadowed cells" % st["shadowed_cells"] in err
    assert "size %d, capacity %d" % (st["base_size"], st["capacity"]) in err and "load %.4f" % st["load"] in err
    ts = st["taxon_stats"]
    assert ts[0]["base_cells"] == 0 < ts[0]["cells"] and ts[1]["cells"] < ts[1]["base_cells"] and ts[2]["base_cells"] == 0 < ts[2]["cells"]
    for x, name in zip(ts, ("root", "the host", "the decoy")):
        line = "%s (taxid %d): %d cells before, %d after" % (name, x["taxid"], x["base_cells"], x["cells"])
        assert line in err, (line, err)
    # without -v: no such lines
    p = subprocess.run([BIN, "--build-db", str(tmp_path / "quiet"), "--extend-db", str(decoy["base"]), "--reference", decoy["fa"], "--taxid", str(DECOY),
                        "--taxon-name", "the decoy"], capture_output=True, timeout=300)
    assert p.returncode == 0 and b"cells before" not in p.stderr and b"cells added" in p.stderr
    assert digest(tmp_path / "quiet")["taxo.k2d"] == digest(d)["taxo.k2d"]
    u.same_table(table(tmp_path / "quiet"), table(d))
