"""Pure-Python model of the per-taxon outputs (nh_run_taxa, `--taxon-out`): which selector a call goes to, and what every
selector's file holds, cut out of the output of a keep_human = 1 run of the same inputs.

A selector is an external taxid or "other".  A classified fragment goes to the deepest selected taxon that is its call or an
ancestor of its call; if none is, to "other" where that was given, else nowhere.  `parent` maps every external taxid of the
taxonomy to its parent's (the root's parent: 0 or absent)."""
import re

OTHER = "other"
SUFFIX = re.compile(rb" kraken:taxid\|(\d+)$")


def parent_map(external_ids, parent):
    """the parent map of a golden file's meta: internal tables -> {external child: external parent}"""
    return {external_ids[i]: (external_ids[parent[i]] if parent[i] else 0) for i in range(1, len(external_ids))}


def bin_of(parent, selectors):
    """{external taxid: selector index or None} for every node of the taxonomy"""
    own = {s: k for k, s in enumerate(selectors) if s != OTHER}
    assert len(own) + (OTHER in selectors) == len(selectors), "a selector twice"
    for s in own:
        assert s in parent, "taxid %r is not in the taxonomy" % (s,)
    other = selectors.index(OTHER) if OTHER in selectors else None
    out = {}
    for node in parent:
        at, seen = node, 0
        while at and at not in own:
            at = parent.get(at, 0)
            seen += 1
            assert seen <= len(parent), "cycle"
        out[node] = own[at] if at else other
    return out


def records(data, fastq):
    """the records of a normalised output (four lines a FASTQ record, two a FASTA record), each with its final newline"""
    lines = data.split(b"\n")
    assert lines[-1] == b"", "the output does not end with a newline"
    per = 4 if fastq else 2
    assert (len(lines) - 1) % per == 0, "not whole records"
    return [b"\n".join(lines[i:i + per]) + b"\n" for i in range(0, len(lines) - 1, per)]


def record_taxid(rec):
    m = SUFFIX.search(rec.split(b"\n", 1)[0])
    assert m, rec[:80]
    return int(m.group(1))


def partition(data, fastq, parent, selectors):
    """(files, counts): the bytes of every selector's file and its records, from a keep_human = 1 output"""
    bins = bin_of(parent, selectors)
    files = [[] for _ in selectors]
    for rec in records(data, fastq):
        k = bins[record_taxid(rec)]
        if k is not None:
            files[k].append(rec)
    return [b"".join(f) for f in files], [len(f) for f in files]


def route_calls(calls, parent, selectors):
    """per selector the indices of the fragments it takes, from the external taxid of every fragment's call (0: unclassified)"""
    bins = bin_of(parent, selectors)
    out = [[] for _ in selectors]
    for i, c in enumerate(calls):
        k = bins[c] if c else None
        if k is not None:
            out[k].append(i)
    return out
