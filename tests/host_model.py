"""Pure-Python model of the host selection (nh_run_host, `--host-taxid` / `--keep-taxid`): which nodes of a taxonomy are host, and
what the outputs that follow the selection hold.  Test helper: it never imports the engine.

Two lists of external taxids, host and keep.  A node is HOST iff the deepest listed taxon that is the node or an ancestor of it
is a host taxid; no listed ancestor: not host.  A classified fragment is a host fragment iff its call is a host node; an
unclassified fragment (call 0) never is; a classified fragment that is not host is SPARED and written as an unclassified one.
`parent` maps every external taxid of the taxonomy to its parent's (the root's parent: 0 or absent), as tests/taxout_model.py.

  host_of            {external taxid: bool} for every node
  is_host            of a fragment's call (0: unclassified)
  table              host_of as the bytes of nh_host_table_image: a byte per internal id, entry 0 is 0
  filter_keep_human  the records of a keep_human = 1 output (a " kraken:taxid|N" suffix on every header) that are host
  normalised         a record (header, sequence, qualities) as the engine writes it, with the suffix of a taxid or without
  kept / removed / masked / ids   the outputs of a run from the input's records and the external taxid of every fragment's call"""
from tests import taxout_model as tm


def host_of(parent, host, keep=()):
    host, keep = list(host), list(keep)
    listed = host + keep
    assert len(set(listed)) == len(listed), "a taxid twice"
    assert 0 not in listed, "taxid 0"
    assert host or not keep, "keep without host"
    for t in listed:
        assert t in parent, "taxid %r is not in the taxonomy" % (t,)
    hs, ks = set(host), set(keep)
    out = {}
    for node in parent:
        at, seen = node, 0
        while at and at not in hs and at not in ks:
            at = parent.get(at, 0)
            seen += 1
            assert seen <= len(parent), "cycle"
        out[node] = bool(at) and at in hs
    return out


def is_host(call, hostmap):
    return bool(call) and hostmap[call]


def table(external_ids, hostmap):
    """external_ids[i]: the external id of internal node i (entry 0: the sentinel)"""
    return bytes([0] + [int(hostmap[e]) for e in external_ids[1:]])


def filter_keep_human(data, fastq, hostmap):
    return b"".join(r for r in tm.records(data, fastq) if is_host(tm.record_taxid(r), hostmap))


def normalised(rec, fastq, taxid=None, mask=False):
    h, seq, qual = rec
    if taxid:
        h = h + b" kraken:taxid|%d" % taxid
    if mask:
        seq = b"N" * len(seq)
    return h + b"\n" + seq + (b"\n+\n" + qual if fastq else b"") + b"\n"


def kept(records, calls, hostmap, fastq):
    """out1 / out2 of a plain run: the fragments that are not host, none with a suffix"""
    return b"".join(normalised(r, fastq) for r, c in zip(records, calls) if not is_host(c, hostmap))


def removed(records, calls, hostmap, fastq):
    """the host fragments as -H / the human outputs write them: the suffix carries the true call"""
    return b"".join(normalised(r, fastq, c) for r, c in zip(records, calls) if is_host(c, hostmap))


def masked(records, calls, hostmap, fastq):
    """every record, N over the host fragments' bases"""
    return b"".join(normalised(r, fastq, mask=is_host(c, hostmap)) for r, c in zip(records, calls))


def ids(names, calls, hostmap):
    return b"".join(n + b"\n" for n, c in zip(names, calls) if is_host(c, hostmap))
