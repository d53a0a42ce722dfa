"""kmer_id_amd -- MI355X-native k-mer read classifier (drop-in for the hot path of
mmammel8/kmer_id's newkmer_10nx.cpp).  The product is the C-ABI library
libkmer_id_amd.so (include/kmer_id_amd.h) and the nk10-compatible CLI; this
package is the thin Python host layer used by the tests, the benchmark and the
multi-GPU launcher.
"""
from ._lib import KidError, KID_FLAG_HOST_BUILD, KID_FLAG_REF_GEOMETRY, KID_FLAG_U_IS_T, KID_OPT_INPUTS_READY, KID_OPT_MIN_BASE_QUALITY, KID_OPT_ENTRY_DEPTH, KID_DB_OPT_MIN_BASE_QUALITY, KID_OPT_LOW_COMPLEXITY, KID_DB_OPT_LOW_COMPLEXITY, KID_OPT_LINE_DIGEST, device_count, load  # noqa: F401
from .api import COVERAGE_DTYPE, FRAGMENT_DTYPE, FRAGMENT_LOCUS_DTYPE, FRAGMENT_VOTE_DTYPE, LOCUS_DTYPE, PILEUP_DTYPE, SEGMENT_DTYPE, SEGMENT_VOTE_DTYPE, VOTE_DTYPE, KmerDB, Pileup, PinnedBuffer, Sample, depth_spectrum_merged, end_merged, hash_keys, read_probe_sites, read_seen_file, seen_coverage, seen_coverage_bins, shared_kmers, write_seen_file  # noqa: F401

__all__ = ["KmerDB", "Sample", "PinnedBuffer", "hash_keys", "end_merged", "depth_spectrum_merged", "shared_kmers", "seen_coverage", "seen_coverage_bins", "read_probe_sites", "COVERAGE_DTYPE", "LOCUS_DTYPE", "FRAGMENT_LOCUS_DTYPE", "PILEUP_DTYPE", "Pileup", "read_seen_file", "write_seen_file", "KidError", "device_count", "load", "KID_FLAG_U_IS_T", "KID_FLAG_HOST_BUILD", "KID_FLAG_REF_GEOMETRY", "KID_OPT_INPUTS_READY", "KID_OPT_MIN_BASE_QUALITY", "KID_OPT_ENTRY_DEPTH", "KID_DB_OPT_MIN_BASE_QUALITY", "KID_OPT_LOW_COMPLEXITY", "KID_DB_OPT_LOW_COMPLEXITY", "KID_OPT_LINE_DIGEST"]
