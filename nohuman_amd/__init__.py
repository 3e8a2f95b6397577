"""nohuman_amd -- MI355X (gfx950) in-process replacement for nohuman's kraken2 subprocess.

Only the classification hot path lives here: HIP kernels + the C ABI of
include/nohuman_engine.h (csrc/), and a thin Python host mirror of the reference's boundary
(`CommandRunner`, /root/reference/src/lib.rs:11-58).  There is no CPU fallback: every entry fails
loudly when libnohuman_engine.so or a gfx950 device is missing.
"""
from .engine import Engine, EngineError, ReadStats, RESULT_DTYPE, probe, device_count, build_db, extend_db, dust_mask, bam_scan, bam_scan_pairs, bam_paired  # noqa: F401
from .engine import CODEC_NONE, CODEC_BZIP2, CODEC_GZIP, CODEC_XZ, CODEC_ZSTD, CODEC_BGZF  # noqa: F401
from .runner import CommandRunner, parse_kraken_stderr, validate_db_directory, \
    parse_confidence_score  # noqa: F401

__all__ = ["Engine", "EngineError", "ReadStats", "RESULT_DTYPE", "probe", "device_count", "build_db", "extend_db", "dust_mask", "bam_scan", "bam_scan_pairs", "bam_paired", "CommandRunner",
           "parse_kraken_stderr", "validate_db_directory", "parse_confidence_score",
           "CODEC_NONE", "CODEC_BZIP2", "CODEC_GZIP", "CODEC_XZ", "CODEC_ZSTD", "CODEC_BGZF"]
