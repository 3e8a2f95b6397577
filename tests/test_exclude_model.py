"""tests/exclude_model.py, the specification of a build with an exclusion list, against the definition read k-mer by k-mer on
tiny inputs (brute_minimizers: no sliding window, no state across k-mers).  CPU only.  tests/test_gpu_build_db_exclude.py holds
nh_build_db_exclude to this model."""
import numpy as np
import pytest

from oracle import k2_literal as lit
from oracle import minidb
from tests import build_db_util as u
from tests import build_forge as bf
from tests import exclude_model as xm
from tests import synth


def brute(seqs):
    out = set()
    for s in seqs:
        out |= xm.brute_minimizers(s)
    return out


@pytest.fixture(params=[0, 1], ids=["last_lmer", "queue"])
def rule(request, monkeypatch):
    """both ambiguity rules: the model follows the one in force, as the library does"""
    monkeypatch.setenv("NOHUMAN_OPT_AMBIGUITY_RULE", str(request.param))
    assert u.rule() == request.param
    return request.param


def pair(seed, shared=120, revcomp=False, n_at=None):
    """a host of two records and an exclusion input of one; the host's first record carries `shared` bases of the exclusion
    record (reverse-complemented, or with an N at n_at of the stretch in the exclusion record only)"""
    rng = np.random.default_rng(seed)
    x = bytearray(synth.random_seq(rng, 400))
    stretch = bytes(x[150:150 + shared])
    if n_at is not None:
        x[150 + n_at] = ord("N")
    a = synth.random_seq(rng, 90) + (synth.revcomp(stretch) if revcomp else stretch) + synth.random_seq(rng, 110)
    return [a, synth.random_seq(rng, 200).lower()], [bytes(x)], stretch


def test_kept_is_h_minus_x(rule):
    host, excl, stretch = pair(1)
    m = xm.model(host, excl)
    H, X = brute(host), brute(excl)
    assert (m["H"], m["X"]) == (H, X)
    assert m["kept"] == H - X and m["excluded"] == H & X and 0 < len(m["excluded"]) < len(H)
    assert xm.brute_minimizers(stretch) <= m["excluded"]  # every k-mer that lies inside the stretch
    assert m["capacity"] == u.default_capacity(len(H - X)) < u.default_capacity(len(H))
    hdr, cells = u.cells_of(m["table"])
    bf.valid_table(hdr, cells, H - X, m["capacity"])
    xm.order_free(m)
    # the table is the one of a host whose minimizers are the kept ones: the excluded are not found, unless they share a key
    assert xm.still_found(cells, m["excluded"], m["capacity"]) == [] == xm.shared_keys(m["kept"], m["excluded"])
    assert (m["x_sequences"], m["x_bases"], m["x_kmers"], m["x_ambiguous"]) == (1, 400, 366, 0)
    assert len(X) <= m["x_lookups"] <= m["x_kmers"]
    # an exclusion input that shares nothing, and none at all: the plain build
    other = [synth.random_seq(np.random.default_rng(99), 300)]
    for x in (other, []):
        p = xm.model(host, x)
        assert p["kept"] == H and not p["excluded"] and p["table"] == u.model_hash(host, p["capacity"])[0]
    # the host as its own exclusion: nothing is left, and no table
    e = xm.model(host, host)
    assert not e["kept"] and e["excluded"] == H and e["table"] is None


def test_a_reverse_complemented_stretch_is_excluded(rule):
    host, excl, stretch = pair(2, revcomp=True)
    assert stretch not in host[0] and synth.revcomp(stretch) in host[0]
    m = xm.model(host, excl)
    inside = xm.brute_minimizers(stretch)
    assert len(inside) > 10 and inside == xm.brute_minimizers(synth.revcomp(stretch))  # (minimizers are canonical)
    assert inside <= m["excluded"] and not inside & m["kept"]
    assert m["kept"] == brute(host) - brute(excl)


@pytest.mark.parametrize("n_at", [0, 3, 4, 34, 35, 60, 115, 116, 119])
def test_an_n_in_the_exclusion_input_spares_what_the_rule_says(rule, n_at):
    """the N sits in the exclusion record only: the k-mers of the host's stretch that the N makes ambiguous THERE keep their
    minimizers (where no other k-mer of the exclusion input has them), and a k-mer that only starts with the N loses one or more
    of its l-mers, not its place"""
    host, excl, stretch = pair(3, n_at=n_at)
    m = xm.model(host, excl)
    whole = xm.model(host, pair(3)[1])
    assert m["kept"] == brute(host) - brute(excl) and m["H"] == whole["H"]
    spared = whole["excluded"] - m["excluded"]
    assert m["kept"] - whole["kept"] == spared
    # only the k-mers that hold the N's position change: what they gave the exclusion set, and no other k-mer of it still gives
    p = 150 + n_at
    around = xm.brute_minimizers(pair(3)[1][0][p - 34:p + 35])
    assert spared == (m["H"] & around) - brute(excl)
    assert spared >= xm.brute_minimizers(stretch) - brute(excl)
    span = 31 if rule == 0 else 34
    # k-mers of the stretch with the N in their last `span` bases are ambiguous: the k-mers at n_at - 34 + (35 - span) .. n_at
    ambiguous = [i for i in range(len(stretch) - 34) if i + 35 - span <= n_at <= i + 34]
    # (a k-mer that only starts with the N is not among them: the first 35 - span bases of a k-mer may be anything)
    assert len(ambiguous) == max(0, min(85, n_at - 35 + span) - max(0, n_at - 34) + 1)
    assert m["x_ambiguous"] == len([i for i in range(366) if i + 35 - span <= 150 + n_at <= i + 34])
    if len(ambiguous) >= 20:
        assert spared, "an N in the middle of the stretch spares something"


def test_the_shared_key_count_on_a_forged_pair():
    """an excluded and a kept minimizer with one compacted key and one home: the table of the kept one answers for both"""
    cap = 61
    rng = np.random.default_rng(4)
    (kept, r_kept), (gone, r_gone), (alone, r_alone) = bf.forge(cap, [(17, 0x12345), (17, 0x12345), (40, 0x54321)], rng)
    assert kept != gone and lit.fmix64(kept) >> bf.KEY_SHIFT == lit.fmix64(gone) >> bf.KEY_SHIFT == 0x12345
    m = xm.model([r_kept, r_gone, r_alone], [r_gone], capacity=cap)
    assert m["kept"] == {kept, alone} and m["excluded"] == {gone}
    assert xm.shared_keys(m["kept"], m["excluded"]) == [gone]
    hdr, cells = u.cells_of(m["table"])
    bf.valid_table(hdr, cells, m["kept"], cap)
    assert m["size"] == 2 and cells[17] == 0x12345 << u.VALUE_BITS | 2
    assert xm.still_found(cells, m["excluded"], cap) == [gone]
    # the same with the lone minimizer excluded: its key is nobody else's, and it is gone
    m = xm.model([r_kept, r_gone, r_alone], [r_alone], capacity=cap)
    assert m["excluded"] == {alone} and xm.shared_keys(m["kept"], m["excluded"]) == []
    hdr, cells = u.cells_of(m["table"])
    assert xm.still_found(cells, m["excluded"], cap) == [] and cells[40] == 0 and m["size"] == 1
    with pytest.raises(AssertionError):
        xm.order_free(m)  # (two kept minimizers with one key: same_table would not be the whole truth)


def test_a_manifest_stores_an_excluded_minimizer_under_no_taxon():
    from tests import build_taxa_util as t
    rng = np.random.default_rng(5)
    both, only_a, ab = (synth.random_seq(rng, 100) for _ in range(3))
    a = synth.random_seq(rng, 150) + both + only_a + ab
    b = both + synth.random_seq(rng, 150) + ab
    tax = t.taxonomy_of(t.TREE_LINES)
    pairs = [(t.A, a), (t.B, b)]
    X = brute([both, only_a])
    blob, size = xm.build_hash(tax, pairs, X, 1009)
    full, _ = t.model(tax, pairs, 1009)
    assert xm.build_hash(tax, pairs, set(), 1009)[0] == full
    db = lit.DB.from_images(minidb.opts_bytes(), tax.to_bytes(), blob)
    for m in brute([both]) | brute([only_a]):
        assert db.get(m) == 0
    for m in brute([ab]) - X:
        assert db.get(m) == tax.internal[t.G]  # shared by A and B alone: their lowest common ancestor
    assert size == len(brute([a, b]) - X)
    fast, size_f = xm.build_hash_fast(tax, pairs, X, 1009)
    assert size_f == size
    u.same_table(u.cells_of(fast), u.cells_of(blob))


def test_the_fast_model_is_the_model(rule):
    """model_fast (the C oracle's scanner, sorted insertion) against model() on an input with N, lowercase, records too short for
    a k-mer and a shared stretch: the same sets, totals and run starts, and the same table up to the order of insertion"""
    rng = np.random.default_rng(6)
    g = u.genome(6, n_seq=2, length=600)
    shared = synth.random_seq(rng, 200)
    host = [g[0][1][:300] + shared + g[0][1][300:], g[1][1], b"ACGT" * 8]
    excl = [synth.random_seq(rng, 34), synth.random_seq(rng, 250) + synth.revcomp(shared)[:150] + b"NN" + synth.random_seq(rng, 90), b""]
    m, f = xm.order_free(xm.model(host, excl)), xm.model_fast(host, excl)
    for k in ("H", "X", "kept", "excluded", "capacity", "size", "kmers", "ambiguous", "x_kmers", "x_ambiguous", "x_sequences", "x_bases",
              "x_lookups"):
        assert m[k] == f[k], k
    assert m["excluded"] and m["ambiguous"] and m["x_ambiguous"]
    u.same_table(u.cells_of(m["table"]), u.cells_of(f["table"]))
