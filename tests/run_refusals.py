"""The table of bad whole-run calls behind tests/test_run_refusals.py and tools/record_run_refusals.py, and the code that makes one
call from a line of it.  A case names its entry by suffix ("" is nh_run, "split" is nh_run_split, ...), then only what differs from
a good single-end run on a.fq.  Paths are written with {d}, the case's directory; the recorded messages carry <TMP> and <DB>.

The directory of every case holds: a.fq and b.fq (one record each), a_ln.fq (a hard link to a.fq), e.txt (an existing regular
file), e_ln.txt (a hard link to e.txt) and r.bam (a BAM of one record).  No case may create a file."""
import ctypes as C
import os

from tests import bam_model as bm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DB = os.path.join(ROOT, "tests", "golden", "toy_db")
GOLDEN = os.path.join(ROOT, "tests", "golden", "run_refusals.json")

# the arguments of each entry behind (args, ...) and in front of stats
SHAPE = {"": (), "split": ("h1", "h2"), "mask": ("h1", "h2"), "ex": ("x",), "minq": ("x", "minq"),
         "rstats": ("x", "minq", "rs_path", "rs_out"), "taxa": ("x", "minq", "rs_path", "rs_out", "outs", "n_outs"),
         "mdata": ("x", "minq", "rs_path", "rs_out", "outs", "n_outs", "md"),
         "host": ("x", "minq", "rs_path", "rs_out", "outs", "n_outs", "md", "hf")}


def case(id, entry, **kw):
    kw.update(id=id, entry=entry)
    return kw


A, B, ALN, E, ELN, O, K, R = "{d}/a.fq", "{d}/b.fq", "{d}/a_ln.fq", "{d}/e.txt", "{d}/e_ln.txt", "{d}/o.fq", "{d}/k.txt", "{d}/r.txt"
PAIRED = dict(in2=B, out2="{d}/o2.fq")
NOPE = "{d}/nope.fq"


def sel(taxid, out1="{d}/t1.fq", out2=None):
    return dict(taxid=taxid, out1=out1, out2=out2)


# ---- refused before any device is touched: the same with and without a GPU
CPU_CASES = [
    # nh_run_split / check_split_args
    case("split-null-args", "split", args=None, h1="{d}/h.fq"),
    case("split-h1-missing", "split"),
    case("split-h1-empty", "split", h1=""),
    case("split-keep-human", "split", h1="{d}/h.fq", args=dict(keep_human=1)),
    case("split-paired-needs-h2", "split", h1="{d}/h.fq", args=PAIRED),
    case("split-h2-without-in2", "split", h1="{d}/h.fq", h2="{d}/h2.fq"),
    case("split-h1-is-h2", "split", h1="{d}/h.fq", h2="{d}/h.fq", args=PAIRED),
    case("split-h1-is-in1-string", "split", h1=A),
    case("split-h1-is-in1-link", "split", h1=ALN),
    case("split-h1-is-out1-not-yet-there", "split", h1=O),
    case("split-h1-is-report-link", "split", h1=ELN, args=dict(report=E)),
    case("split-h2-is-in2-link", "split", h1="{d}/h.fq", h2=ALN, args=dict(in2=A, out2="{d}/o2.fq")),
    case("split-empty-h2-is-empty-in2", "split", h1="{d}/h.fq", h2="", args=dict(in2="", out2="{d}/o2.fq")),
    # nh_run_mask / check_mask_args
    case("mask-null-args", "mask", args=None),
    case("mask-keep-human", "mask", args=dict(keep_human=1)),
    case("mask-h2-alone", "mask", h2="{d}/h2.fq"),
    case("mask-h1-keep-human", "mask", h1="{d}/h.fq", args=dict(keep_human=2)),
    case("mask-paired-needs-h2", "mask", h1="{d}/h.fq", args=PAIRED),
    case("mask-h1-is-in1-link", "mask", h1=ALN),
    case("mask-h1-is-kraken", "mask", h1=K),
    case("mask-out1-is-in1-string", "mask", args=dict(out1=A)),
    case("mask-out1-is-in1-link", "mask", args=dict(out1=ALN)),
    case("mask-out1-is-in1-neither-there", "mask", args=dict(in1=NOPE, out1=NOPE)),
    case("mask-report-is-in2-link", "mask", args=dict(in2=E, out2="{d}/o2.fq", report=ELN)),
    case("mask-split-error-before-out-is-in", "mask", h1=A, args=dict(out1=A)),
    # nh_run_ex / check_extras, check_list_args
    case("ex-null-args", "ex", args=None, x=dict()),
    case("ex-null-args-and-extras", "ex", args=None),
    case("ex-null-extras", "ex"),
    case("ex-struct-size", "ex", x=dict(struct_size=39, calls=A)),
    case("ex-split-reports-as-split", "ex", x=dict(human_out1="{d}/h.fq"), args=dict(keep_human=1)),
    case("ex-h2-alone", "ex", x=dict(human_out2="{d}/h2.fq")),
    case("ex-mask-reports-as-mask", "ex", x=dict(mask=1), args=dict(keep_human=1)),
    case("ex-mask-out-is-in", "ex", x=dict(mask=1, calls=A), args=dict(out1=ALN)),
    case("ex-calls-empty", "ex", x=dict(calls="")),
    case("ex-ids-empty", "ex", x=dict(human_ids="")),
    case("ex-calls-is-in1-string", "ex", x=dict(calls=A)),
    case("ex-calls-is-in1-link", "ex", x=dict(calls=ALN)),
    case("ex-calls-is-out1-not-yet-there", "ex", x=dict(calls=O)),
    case("ex-ids-is-in2", "ex", x=dict(human_ids=B), args=PAIRED),
    case("ex-ids-is-h1", "ex", x=dict(human_out1="{d}/h.fq", human_ids="{d}/h.fq")),
    case("ex-ids-is-report-link", "ex", x=dict(human_ids=ELN), args=dict(report=E)),
    case("ex-ids-is-calls-string", "ex", x=dict(calls="{d}/c.txt", human_ids="{d}/c.txt")),
    case("ex-ids-is-calls-link", "ex", x=dict(calls=E, human_ids=ELN)),
    case("ex-split-error-before-list-error", "ex", x=dict(human_out1=A, calls=A)),
    case("ex-mask-error-before-list-error", "ex", x=dict(mask=1, calls=A), args=dict(keep_human=1)),
    # nh_run_minq / check_minq
    case("minq-94", "minq", minq=94),
    case("minq-before-extras", "minq", minq=4000000000, x=dict(struct_size=8)),
    case("minq-extras-struct-size", "minq", minq=93, x=dict(struct_size=0)),
    case("minq-extras-list", "minq", x=dict(calls=A)),
    # nh_run_rstats / check_rstats_args
    case("rstats-null-args", "rstats", args=None, rs_path="{d}/s.tsv"),
    case("rstats-empty", "rstats", rs_path=""),
    case("rstats-is-in1-string", "rstats", rs_path=A),
    case("rstats-is-in1-link", "rstats", rs_path=ALN),
    case("rstats-is-calls-not-yet-there", "rstats", rs_path="{d}/c.txt", x=dict(calls="{d}/c.txt")),
    case("rstats-is-kraken-link", "rstats", rs_path=ELN, args=dict(kraken_output=E)),
    case("rstats-is-h2", "rstats", rs_path="{d}/h2.fq", x=dict(human_out1="{d}/h.fq", human_out2="{d}/h2.fq"), args=PAIRED),
    case("rstats-minq-before-rstats", "rstats", minq=94, rs_path=""),
    case("rstats-extras-before-rstats", "rstats", rs_path=A, x=dict(calls=A)),
    # nh_run_taxa / check_taxon_args
    case("taxa-null-args", "taxa", args=None, outs=[sel(10)]),
    case("taxa-too-many", "taxa", outs=[sel(10)], n_outs=9),
    case("taxa-null-outs", "taxa", outs=None, n_outs=2),
    case("taxa-keep-human", "taxa", outs=[sel(10)], args=dict(keep_human=1)),
    case("taxa-out1-missing", "taxa", outs=[sel(10), sel(20, out1=None)]),
    case("taxa-out1-empty", "taxa", outs=[sel(10, out1="")]),
    case("taxa-out2-empty", "taxa", outs=[sel(10, out2="")], args=PAIRED),
    case("taxa-paired-needs-out2", "taxa", outs=[sel(10)], args=PAIRED),
    case("taxa-out2-without-in2", "taxa", outs=[sel(10, out2="{d}/t2.fq")]),
    case("taxa-other-twice", "taxa", outs=[sel(0), sel(10, out1="{d}/u.fq"), sel(0, out1="{d}/v.fq")]),
    case("taxa-taxid-twice", "taxa", outs=[sel(9606), sel(9606, out1="{d}/u.fq")]),
    case("taxa-out1-is-in1-string", "taxa", outs=[sel(10, out1=A)]),
    case("taxa-out1-is-in1-link", "taxa", outs=[sel(10), sel(20, out1=ALN)]),
    case("taxa-out1-is-rstats-not-yet-there", "taxa", rs_path="{d}/s.tsv", outs=[sel(10, out1="{d}/s.tsv")]),
    case("taxa-out2-is-out2", "taxa", outs=[sel(10, out2="{d}/o2.fq")], args=PAIRED),
    case("taxa-out1-is-ids-link", "taxa", outs=[sel(10, out1=ELN)], x=dict(human_ids=E)),
    case("taxa-out1-is-other-out1-string", "taxa", outs=[sel(10), sel(20)]),
    case("taxa-out2-is-own-out1", "taxa", outs=[sel(10, out2="{d}/t1.fq")], args=PAIRED),
    case("taxa-out1-is-other-out2-link", "taxa", outs=[sel(10, out2=E), sel(20, out1=ELN, out2="{d}/u2.fq")], args=PAIRED),
    case("taxa-rstats-before-taxa", "taxa", rs_path=A, outs=[sel(10, out1=A)]),
    # nh_run_mdata / check_mdata_args
    case("mdata-struct-size", "mdata", md=dict(struct_size=31, in_report=1)),
    case("mdata-struct-size-before-null-args", "mdata", args=None, md=dict(struct_size=0)),
    case("mdata-null-args", "mdata", args=None, md=dict(in_report=1)),
    case("mdata-in-report-without-report", "mdata", md=dict(in_report=1), args=dict(report=None)),
    case("mdata-in-report-with-empty-report", "mdata", md=dict(in_report=1), args=dict(report="")),
    case("mdata-taxa-cap-0", "mdata", md=dict(taxa=True, taxa_cap=0)),
    case("mdata-table-empty", "mdata", md=dict(table="")),
    case("mdata-table-is-in1-string", "mdata", md=dict(table=A)),
    case("mdata-table-is-in1-link", "mdata", md=dict(table=ALN)),
    case("mdata-table-is-rstats-not-yet-there", "mdata", rs_path="{d}/s.tsv", md=dict(table="{d}/s.tsv")),
    case("mdata-table-is-selector-out1", "mdata", outs=[sel(10)], md=dict(table="{d}/t1.fq")),
    case("mdata-table-is-report-link", "mdata", md=dict(table=ELN), args=dict(report=E)),
    case("mdata-table-is-calls", "mdata", x=dict(calls="{d}/c.txt"), md=dict(table="{d}/c.txt")),
    case("mdata-taxa-before-mdata", "mdata", outs=[sel(10, out1=A)], md=dict(table=A)),
    # nh_run_host / check_host_filter
    case("host-struct-size", "host", hf=dict(host=[9606], size=47)),
    case("host-keep-without-host", "host", hf=dict(keep=[9606])),
    case("host-too-many", "host", hf=dict(host=list(range(2, 12)), keep=list(range(12, 19)))),
    case("host-null-host-list", "host", hf=dict(host=[9606], null_host=True)),
    case("host-null-keep-list", "host", hf=dict(host=[9606], keep=[10], null_keep=True)),
    case("host-taxid-0-host", "host", hf=dict(host=[9606, 0])),
    case("host-taxid-0-keep", "host", hf=dict(host=[9606], keep=[0])),
    case("host-taxid-twice", "host", hf=dict(host=[1, 9606], keep=[9606])),
    case("host-before-minq", "host", hf=dict(keep=[9606]), minq=94),
    case("host-then-mdata-checks", "host", hf=dict(host=[9606]), md=dict(struct_size=31)),
    case("host-no-selection-is-mdata", "host", hf=dict(), md=dict(struct_size=31)),
    case("host-null-is-mdata", "host", md=dict(table=A)),
    # behind the argument errors: the null engine / the missing db_dir, then the BAM inputs (the two entries differ from here on)
    case("args-before-engine-and-db", "minq", minq=94, args=dict(db_dir=None)),
    case("run-null-args", "", args=None, same=False),
    case("minq-null-args-nothing-asked", "minq", args=None, same=False),
    case("rstats-null-args-nothing-asked", "rstats", args=None, x=None, same=False),
    case("run-no-db", "", args=dict(db_dir=None), same=False),
    case("split-empty-h2-beside-empty-report-passes", "split", h1="{d}/h.fq", h2="", args=dict(db_dir=None, in2=B, out2="{d}/o2.fq", report=""), same=False),
    case("db-before-bam", "", args=dict(db_dir=None, in2="{d}/r.bam", out2="{d}/o2.fq"), same=False),
    case("bam-in2", "", args=dict(in2="{d}/r.bam", out2="{d}/o2.fq"), same=False),
    case("bam-in1-beside-in2", "host", args=dict(in1="{d}/r.bam", in2=B, out2="{d}/o2.fq"), hf=dict(host=[9606]), same=False),
    case("bam-in2-split", "split", h1="{d}/h.fq", h2="{d}/h2.fq", args=dict(in2="{d}/r.bam", out2="{d}/o2.fq"), same=False),
]

# ---- refused by the run itself, the database open: against tests/golden/toy_db with an engine, before the first kernel
GPU_CASES = [
    case("run-paired-without-out2", "", args=dict(in2=B)),
    case("run-confidence-1.5", "", args=dict(confidence=1.5)),
    case("run-out-codec-99", "", args=dict(out_codec=99)),
    case("run-in1-missing", "", args=dict(in1=NOPE)),
    case("run-out1-is-in1-link", "", args=dict(out1=ALN)),
    case("taxa-taxid-not-in-taxonomy", "taxa", outs=[sel(424242)]),
    case("host-taxid-not-in-taxonomy", "host", hf=dict(host=[9606, 434343])),
]


def make_files(d):
    """the directory of one case -> the sorted names in it"""
    with open(os.path.join(d, "a.fq"), "wb") as f:
        f.write(b"@r\nACGT\n+\nIIII\n")
    with open(os.path.join(d, "b.fq"), "wb") as f:
        f.write(b"@r\nTTGA\n+\nIIII\n")
    with open(os.path.join(d, "e.txt"), "wb") as f:
        f.write(b"here before the run\n")
    os.link(os.path.join(d, "a.fq"), os.path.join(d, "a_ln.fq"))
    os.link(os.path.join(d, "e.txt"), os.path.join(d, "e_ln.txt"))
    with open(os.path.join(d, "r.bam"), "wb") as f:
        f.write(bm.bgzf(bm.forge_header() + bm.forge_record(b"r1", b"ACGTACGT", bytes(8))))
    return sorted(os.listdir(d))


def _s(v, d):
    return None if v is None else v.replace("{d}", d).encode()


def call(L, c, d, engine):
    """one case through its standalone entry (engine False) or its engine twin (engine None: no engine, else the handle)
    -> [code, message with <TMP> and <DB>]"""
    from nohuman_amd import _lib
    keep = []  # what the structs point to
    a = None
    if c.get("args", {}) is not None:
        a = _lib.nh_run_args()
        f = dict(db_dir=DB, in1=A, out1=O, kraken_output=K, report=R, n_devices=1)
        f.update(c.get("args", {}))
        for k, v in f.items():
            setattr(a, k, _s(v, d) if isinstance(v, str) or v is None else v)
    x = None
    if c.get("x") is not None:
        xs = dict(c["x"])
        x = _lib.nh_run_extras(struct_size=xs.pop("struct_size", C.sizeof(_lib.nh_run_extras)), mask=xs.pop("mask", 0))
        for k, v in xs.items():
            setattr(x, k, _s(v, d))
    outs = None
    if c.get("outs") is not None:
        outs = (_lib.nh_taxon_out * len(c["outs"]))()
        for o, s in zip(outs, c["outs"]):
            o.taxid, o.out1, o.out2 = s["taxid"], _s(s["out1"], d), _s(s["out2"], d)
    md = None
    if c.get("md") is not None:
        m = c["md"]
        md = _lib.nh_minimizer_data(struct_size=m.get("struct_size", C.sizeof(_lib.nh_minimizer_data)), in_report=m.get("in_report", 0),
                                    table=_s(m.get("table"), d), taxa_cap=m.get("taxa_cap", 0))
        if m.get("taxa"):
            keep.append((_lib.nh_taxon_minimizers * 4)())
            md.taxa = keep[-1]
    hf = None
    if c.get("hf") is not None:
        h = c["hf"]
        host, keeps = h.get("host", []), h.get("keep", [])
        hf = _lib.nh_host_filter(struct_size=h.get("size", C.sizeof(_lib.nh_host_filter)), n_host=len(host), n_keep=len(keeps))
        keep += [(C.c_uint64 * max(len(host), 1))(*host), (C.c_uint64 * max(len(keeps), 1))(*keeps)]
        if not h.get("null_host"):
            hf.host_taxids = keep[-2]
        if not h.get("null_keep"):
            hf.keep_taxids = keep[-1]
    ref = lambda s: C.byref(s) if s is not None else None
    value = dict(h1=_s(c.get("h1"), d), h2=_s(c.get("h2"), d), x=ref(x), minq=c.get("minq", 0), rs_path=_s(c.get("rs_path"), d), rs_out=None,
                 outs=outs, n_outs=c.get("n_outs", len(c["outs"]) if c.get("outs") else 0), md=ref(md), hf=ref(hf))
    stats = _lib.nh_stats()
    entry = c["entry"]
    name = ("nh_run" if engine is False else "nh_run_engine") + ("_" + entry if entry else "")
    pre = () if engine is False else (engine,)
    rc = getattr(L, name)(*pre, ref(a), *[value[k] for k in SHAPE[entry]], C.byref(stats))
    msg = L.nh_last_error().decode() if rc else ""
    return [rc, msg.replace(d, "<TMP>").replace(DB, "<DB>")]
