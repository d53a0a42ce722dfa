"""Host-side objects over the C ABI: KmerDB (hash table + taxonomy resident in HBM)
and Sample (per-sample gcount / seen-bitmap), mirroring the state the reference
keeps in globals (`ht`, `taxonomy`, `gcount`, `ucount`, `kmer_seen`,
newkmer_10nx.cpp:59-64,156,266).  numpy arrays in, numpy arrays out.
"""
import ctypes as C
import struct

import numpy as np

from . import _lib
from ._lib import KidDbInfo, check


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _as(a, dtype):
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=dtype)
    return a


def _offsets_batch(bases, offsets, start, stop):
    """a batch of reads as the C ABI takes it -> (bases, offsets, start, stop, n)"""
    offsets = _as(offsets, np.uint64)
    return _as(bases, np.uint8), offsets, _as(start, np.int32), _as(stop, np.int32), offsets.size - 1


def _fastq_block(text, recs):
    """a block of FASTQ text (bytes or an array) and its line index as the C ABI takes them -> (text, recs, n)"""
    text = _as(np.frombuffer(text, np.uint8) if isinstance(text, (bytes, bytearray)) else text, np.uint8)
    recs = _as(recs, np.uint32).reshape(-1, 4)
    return text, recs, recs.shape[0]


def hash_keys(keys, device=0):
    """Hashtable::integerHash (fmix64) of every key, computed on the GPU."""
    lib = _lib.load()
    keys = _as(keys, np.uint64)
    out = np.empty(keys.size, np.uint64)
    check(lib.kid_hash_keys(device, _ptr(keys), keys.size, _ptr(out)))
    return out


class PinnedBuffer:
    """Page-locked host memory from the library (kid_host_alloc), viewed as a numpy array."""

    def __init__(self, nbytes, device=0):
        self._lib = _lib.load()
        p = C.c_void_p()
        check(self._lib.kid_host_alloc(device, nbytes, C.byref(p)))
        self.ptr = p.value
        self.nbytes = nbytes
        self.array = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), (nbytes,))

    def close(self):
        if getattr(self, "ptr", None):
            self.array = None
            self._lib.kid_host_free(C.c_void_p(self.ptr))
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ReadHits:
    """Every read's k-mer hits in read-position order (kid_db_read_hits*): CSR `offsets` (uint64[n + 1]) over the
    parallel uint32 arrays `pos`, `target`, `entry`, and `n_kmers` (uint32[n]: windows looked up per read)."""

    def __init__(self, offsets, n_kmers, hits):
        self.offsets = offsets
        self.n_kmers = n_kmers
        hits = hits.reshape(-1, 3)
        self.pos = np.ascontiguousarray(hits[:, 0])
        self.target = np.ascontiguousarray(hits[:, 1])
        self.entry = np.ascontiguousarray(hits[:, 2])

    def __len__(self):
        return self.offsets.size - 1

    def of(self, r):
        """-> (pos, target, entry) of read r"""
        a, b = int(self.offsets[r]), int(self.offsets[r + 1])
        return self.pos[a:b], self.target[a:b], self.entry[a:b]


# kid_support: one record per read (kid_db_read_support*)
SUPPORT_DTYPE = np.dtype([("final", np.uint32), ("confident", np.uint32), ("n_kmers", np.uint32), ("n_hits", np.uint32),
                          ("s_final", np.uint32), ("s_confident", np.uint32)])

# kid_fragment: one record per fragment (kid_db_read_fragments*); the first six fields are SUPPORT_DTYPE's
FRAGMENT_DTYPE = np.dtype([(name, np.uint32) for name in SUPPORT_DTYPE.names] + [("final_1", np.uint32), ("final_2", np.uint32)])

# kid_vote: one record per read (kid_db_read_votes*)
VOTE_DTYPE = np.dtype([("call", np.uint32), ("confident", np.uint32), ("n_kmers", np.uint32), ("n_hits", np.uint32),
                       ("p_best", np.uint32), ("n_best", np.uint32), ("s_call", np.uint32), ("s_confident", np.uint32)])

# kid_fragment_vote: one record per fragment (kid_db_read_fragment_votes*); the first eight fields are VOTE_DTYPE's
FRAGMENT_VOTE_DTYPE = np.dtype([(name, np.uint32) for name in VOTE_DTYPE.names] + [("call_1", np.uint32), ("call_2", np.uint32)])

# kid_segment: one record per segment (kid_db_read_segments*); the six fields behind n_pos are SUPPORT_DTYPE's
SEGMENT_DTYPE = np.dtype([("pos", np.uint32), ("n_pos", np.uint32)] + [(name, np.uint32) for name in SUPPORT_DTYPE.names])

# kid_segment_vote: one record per segment (kid_db_read_segment_votes*); the eight fields behind n_pos are VOTE_DTYPE's
SEGMENT_VOTE_DTYPE = np.dtype([("pos", np.uint32), ("n_pos", np.uint32)] + [(name, np.uint32) for name in VOTE_DTYPE.names])

# kid_locus: one record per read (kid_db_read_loci*)
LOCUS_DTYPE = np.dtype([(name, np.uint32) for name in ("org", "strand", "n_chain", "n_org", "n_other", "n_hits", "n_kmers", "pos_first",
                                                       "pos_last", "entry_first")])
# kid_fragment_locus: one record per fragment (kid_db_read_fragment_loci*): sixteen uint32
FRAGMENT_LOCUS_DTYPE = np.dtype([(name, np.uint32) for name in ("org", "orient", "mates", "n_chain", "n_chain_1", "n_chain_2", "n_org", "n_other",
                                                                "n_hits", "n_kmers", "lo", "hi", "pos_first_1", "pos_last_1", "pos_first_2",
                                                                "pos_last_2")])
# kid_pileup_rec: one record per organism (kid_pileup_summary): nine uint32, four bytes of padding, depth_sum at offset 40
PILEUP_FIELDS = ("n_placed", "span_bins", "bins_covered", "max_gap", "max_depth", "max_depth_bin", "max_starts", "max_starts_bin", "reserved")
PILEUP_DTYPE = np.dtype({"names": PILEUP_FIELDS + ("depth_sum",), "formats": [np.uint32] * 9 + [np.uint64],
                         "offsets": [4 * i for i in range(9)] + [40], "itemsize": 48})


# the families of calls over the hit pass by the name in their entry points: the record, and for those that leave one
# record per unit the reads of a unit
_UNIT_FAMILIES = {"support": (SUPPORT_DTYPE, 1), "votes": (VOTE_DTYPE, 1), "fragments": (FRAGMENT_DTYPE, 2),
                  "fragment_votes": (FRAGMENT_VOTE_DTYPE, 2)}
_SEGMENT_FAMILIES = {"segments": SEGMENT_DTYPE, "segment_votes": SEGMENT_VOTE_DTYPE}
# the families that place by the database's sites: their parameters are (diag_bin,) and (diag_bin, max_span)
_LOCI_FAMILIES = {"loci": (LOCUS_DTYPE, 1), "fragment_loci": (FRAGMENT_LOCUS_DTYPE, 2)}


class ReadSegments:
    """Every read's segments in read order (kid_db_read_segments*, kid_db_read_segment_votes*): CSR `offsets`
    (uint64[n + 1]) over `records` (SEGMENT_DTYPE, SEGMENT_VOTE_DTYPE).  The list is dense: segments without a hit are
    there, with final = confident = 0 (call = confident = 0)."""

    def __init__(self, offsets, records):
        self.offsets = offsets
        self.records = records

    def __len__(self):
        return self.offsets.size - 1

    def of(self, r):
        """-> the records of read r"""
        return self.records[int(self.offsets[r]):int(self.offsets[r + 1])]


class KmerDB:
    """Replaces `new Hashtable()` + `new Tree1()` + the add_kmer/add_edge load loops."""

    def __init__(self, keys, targets, parent, k=30, log2_slots=30, max_probes=0, flags=0, device=0):
        lib = _lib.load()
        keys = _as(keys, np.uint64)
        targets = _as(targets, np.uint32)
        parent = _as(parent, np.int32)
        if keys.shape != targets.shape or keys.ndim != 1:
            raise ValueError("keys and targets must be 1-D arrays of equal length")
        h = C.c_void_p()
        check(lib.kid_db_build(_ptr(keys), _ptr(targets), keys.size, _ptr(parent), parent.size, k, log2_slots,
                               max_probes, flags, device, C.byref(h)))
        self._h = h
        self._lib = lib

    @classmethod
    def from_device(cls, d_keys, d_targets, n, parent, k=30, log2_slots=30, max_probes=0, flags=0, device=0):
        """keys/targets already in HBM (raw device pointers, e.g. torch .data_ptr())."""
        lib = _lib.load()
        parent = _as(parent, np.int32)
        self = cls.__new__(cls)
        h = C.c_void_p()
        check(lib.kid_db_build_device(C.c_void_p(d_keys), C.c_void_p(d_targets), n, _ptr(parent), parent.size, k,
                                      log2_slots, max_probes, flags, device, C.byref(h)))
        self._h = h
        self._lib = lib
        return self

    def replicate(self, device):
        """A replica of this database in the HBM of `device` (device-to-device copies)."""
        other = KmerDB.__new__(KmerDB)
        h = C.c_void_p()
        check(self._lib.kid_db_replicate(self._h, device, C.byref(h)))
        other._h = h
        other._lib = self._lib
        return other

    @property
    def info(self):
        out = KidDbInfo()
        check(self._lib.kid_db_get_info(self._h, C.byref(out)))
        return out

    def lookup(self, keys, with_probes=False):
        """Hashtable::getHash for a batch of keys (newkmer_10nx.cpp:204-233)."""
        keys = _as(keys, np.uint64)
        targets = np.empty(keys.size, np.uint32)
        probes = np.empty(keys.size, np.uint32) if with_probes else None
        check(self._lib.kid_db_lookup(self._h, _ptr(keys), keys.size, _ptr(targets), _ptr(probes)))
        return (targets, probes) if with_probes else targets

    def msca(self, x, y):
        """Tree1::msca for a batch of pairs (newkmer_10nx.cpp:118-144)."""
        x = _as(x, np.int32)
        y = _as(y, np.int32)
        out = np.empty(x.size, np.int32)
        check(self._lib.kid_db_msca(self._h, _ptr(x), _ptr(y), x.size, _ptr(out)))
        return out

    def trim(self, quals, offsets):
        """process_qual for a batch (newkmer_10nx.cpp:714-760) -> (start, stop, keep)."""
        quals = _as(quals, np.uint8)
        offsets = _as(offsets, np.uint64)
        n = offsets.size - 1
        start = np.empty(n, np.int32)
        stop = np.empty(n, np.int32)
        keep = np.empty(n, np.uint8)
        check(self._lib.kid_trim_batch(self._h, _ptr(quals), _ptr(offsets), n, _ptr(start), _ptr(stop), _ptr(keep)))
        return start, stop, keep

    def set_option(self, option, value):
        """kid_db_set_option, e.g. (KID_DB_OPT_MIN_BASE_QUALITY, Q): read_hits_fastq and read_support_fastq read every
        base of quality below Q as 'N'; (KID_DB_OPT_LOW_COMPLEXITY, T): ... every base of a low-complexity window."""
        check(self._lib.kid_db_set_option(self._h, option, value))

    def mask_low_quality(self, bases, quals, offsets, q):
        """Bases whose quality byte (quals laid out like bases), read as signed char, is below q + 33 become 'N'
        (kid_mask_batch) -> (masked copy of bases, number of bases masked).  q = 0: the text as it is and 0."""
        bases = _as(bases, np.uint8)
        quals = _as(quals, np.uint8)
        offsets = _as(offsets, np.uint64)
        out = bases.copy()
        n_masked = C.c_uint64(0)
        check(self._lib.kid_mask_batch(self._h, _ptr(bases), _ptr(quals), _ptr(offsets), offsets.size - 1, q, _ptr(out),
                                       C.byref(n_masked)))
        return out, n_masked.value

    def mask_low_quality_device(self, d_bases, d_quals, d_offsets, n_reads, q, d_n_masked=0, stream=0):
        """The same in place on text resident in HBM (raw pointers), asynchronous on `stream`: kid_mask_batch_device.
        d_n_masked: one uint64 in HBM that the number of bases masked is added to (or 0)."""
        check(self._lib.kid_mask_batch_device(self._h, C.c_void_p(d_bases), C.c_void_p(d_quals), C.c_void_p(d_offsets), n_reads, q,
                                              C.c_void_p(d_n_masked or None), C.c_void_p(stream or None)))

    def mask_low_complexity(self, bases, offsets, t):
        """Bases that lie in a low-complexity window at threshold t (0..1000; the rule: kmer_id_amd.h, "mask low-complexity
        sequence") become 'N', read by read (kid_lowc_batch) -> (masked copy of bases, number of bases masked).  t = 0: the
        text as it is and 0."""
        bases = _as(bases, np.uint8)
        offsets = _as(offsets, np.uint64)
        out = bases.copy()
        n_masked = C.c_uint64(0)
        check(self._lib.kid_lowc_batch(self._h, _ptr(bases), _ptr(offsets), offsets.size - 1, t, _ptr(out), C.byref(n_masked)))
        return out, n_masked.value

    def mask_low_complexity_device(self, d_bases, d_offsets, n_reads, t, d_n_masked=0, stream=0):
        """The same in place on text resident in HBM (raw pointers), asynchronous on `stream`: kid_lowc_batch_device.
        d_n_masked: one uint64 in HBM that the number of bases masked is added to (or 0)."""
        check(self._lib.kid_lowc_batch_device(self._h, C.c_void_p(d_bases), C.c_void_p(d_offsets), n_reads, t,
                                              C.c_void_p(d_n_masked or None), C.c_void_p(stream or None)))

    def _read_hits(self, call, n):
        """the sizing call, then the call that fills a buffer of exactly that size"""
        offsets = np.empty(n + 1, np.uint64)
        n_kmers = np.empty(n, np.uint32)
        total = C.c_uint64(0)
        check(call(_ptr(offsets), _ptr(n_kmers), None, 0, C.byref(total)))
        hits = np.empty(total.value * 3, np.uint32)
        if total.value:
            check(call(_ptr(offsets), _ptr(n_kmers), _ptr(hits), total.value, C.byref(total)))
        return ReadHits(offsets, n_kmers, hits)

    def read_hits(self, bases, offsets, start=None, stop=None):
        """The k-mer hits of every read of a batch held in host memory (what process_read folds, newkmer_10nx.cpp:526-595),
        in read-position order -> ReadHits.  Pure: no sample is touched."""
        bases, offsets, start, stop, n = _offsets_batch(bases, offsets, start, stop)
        return self._read_hits(lambda o, nk, h, cap, tot: self._lib.kid_db_read_hits(
            self._h, _ptr(bases), _ptr(offsets), _ptr(start), _ptr(stop), n, o, nk, h, cap, tot), n)

    def read_hits_fastq(self, text, recs):
        """The same for a block of FASTQ text with its line index (uint32[n, 4], as Sample.classify_fastq): process_qual
        runs on the GPU; a record that fails stop - start >= k has no window and no hit."""
        text, recs, n = _fastq_block(text, recs)
        return self._read_hits(lambda o, nk, h, cap, tot: self._lib.kid_db_read_hits_fastq(
            self._h, _ptr(text), text.size, _ptr(recs), n, o, nk, h, cap, tot), n)

    def read_hits_device(self, d_bases, bases_nbytes, d_offsets, n_reads, d_hit_offsets, d_n_hits, d_start=0, d_stop=0,
                         d_n_kmers=0, d_hits=0, cap=0, stream=0):
        """Asynchronous, everything resident in HBM (raw pointers): kid_db_read_hits_device."""
        check(self._lib.kid_db_read_hits_device(self._h, C.c_void_p(d_bases), bases_nbytes, C.c_void_p(d_offsets),
                                                C.c_void_p(d_start or None), C.c_void_p(d_stop or None), n_reads,
                                                C.c_void_p(d_hit_offsets), C.c_void_p(d_n_kmers or None),
                                                C.c_void_p(d_hits or None), cap, C.c_void_p(d_n_hits),
                                                C.c_void_p(stream or None)))

    def _time(self, query):
        ms, calls, reads = C.c_double(0), C.c_uint64(0), C.c_uint64(0)
        check(query(self._h, C.byref(ms), C.byref(calls), C.byref(reads)))
        return ms.value, calls.value, reads.value

    def read_hits_time(self):
        """-> (device ms, calls, reads) of the hits kernels since the last query (HIP events around every call)"""
        return self._time(self._lib.kid_db_read_hits_time)

    def _calls_offsets(self, family, bases, offsets, start, stop, min_hits, min_permille, tally):
        """kid_db_read_<family> over a batch held in host memory -> its records, one per unit"""
        dtype, unit = _UNIT_FAMILIES[family]
        bases, offsets, start, stop, n = _offsets_batch(bases, offsets, start, stop)
        out = np.zeros(n // unit, dtype)
        check(getattr(self._lib, "kid_db_read_" + family)(self._h, _ptr(bases), _ptr(offsets), _ptr(start), _ptr(stop), n, min_hits,
                                                          min_permille, _ptr(out), tally._h if tally is not None else None))
        return out

    def _calls_fastq(self, family, blocks, min_hits, min_permille, tally):
        """kid_db_read_<family>_fastq over one block (text, recs) of FASTQ text, or two: the mates -> one record per unit"""
        blocks = [_fastq_block(text, recs) for text, recs in blocks]
        n = blocks[0][2]
        if any(b[2] != n for b in blocks):
            raise ValueError("recs1 and recs2 must hold one record per fragment each")
        out = np.zeros(n, _UNIT_FAMILIES[family][0])
        texts = [a for text, recs, _ in blocks for a in (_ptr(text), text.size, _ptr(recs))]
        check(getattr(self._lib, "kid_db_read_%s_fastq" % family)(self._h, *texts, n, min_hits, min_permille, _ptr(out),
                                                                  tally._h if tally is not None else None))
        return out

    def _from_hits_device(self, family, d_hit_offsets, d_hits, d_n_kmers, n_reads, d_out, min_hits, min_permille, stream):
        """kid_db_<family>_from_hits_device: a family's kernels alone on a CSR resident in HBM"""
        check(getattr(self._lib, "kid_db_%s_from_hits_device" % family)(
            self._h, C.c_void_p(d_hit_offsets), C.c_void_p(d_hits or None), C.c_void_p(d_n_kmers), n_reads, min_hits, min_permille,
            C.c_void_p(d_out), C.c_void_p(stream or None)))

    def read_support(self, bases, offsets, start=None, stop=None, min_hits=0, min_permille=0, tally=None):
        """Call the reads of a batch held in host memory by k-mer support (kid_db_read_support): -> a structured array
        (SUPPORT_DTYPE: final, confident, n_kmers, n_hits, s_final, s_confident), one record per read.  `confident` is
        the first node on final's root path whose clade holds at least min_hits hits and min_permille / 1000 of the
        read's k-mers, 0 if none does.  tally: a Sample of this database that is counted as if the batch had been
        classified under the rule (gcount[confident]++, seen bits of the hits of reads with confident > 0)."""
        return self._calls_offsets("support", bases, offsets, start, stop, min_hits, min_permille, tally)

    def read_support_fastq(self, text, recs, min_hits=0, min_permille=0, tally=None):
        """The same for a block of FASTQ text with its line index (uint32[n, 4], as Sample.classify_fastq): a record that
        fails stop - start >= k has no window and no hit, and a tally counts it nowhere."""
        return self._calls_fastq("support", [(text, recs)], min_hits, min_permille, tally)

    def support_from_hits_device(self, d_hit_offsets, d_hits, d_n_kmers, n_reads, d_out, min_hits=0, min_permille=0, stream=0):
        """The support kernel alone on a CSR resident in HBM (raw pointers, as kid_db_read_hits_device left it);
        asynchronous on `stream`: kid_db_support_from_hits_device.  d_out: kid_support[n_reads] (SUPPORT_DTYPE)."""
        self._from_hits_device("support", d_hit_offsets, d_hits, d_n_kmers, n_reads, d_out, min_hits, min_permille, stream)

    def read_support_time(self):
        """-> (device ms, calls, reads) of the support kernel alone since the last query"""
        return self._time(self._lib.kid_db_read_support_time)

    def read_votes(self, bases, offsets, start=None, stop=None, min_hits=0, min_permille=0, tally=None):
        """Call the reads of a batch held in host memory by root-path votes (kid_db_read_votes): -> a structured array
        (VOTE_DTYPE: call, confident, n_kmers, n_hits, p_best, n_best, s_call, s_confident), one record per read.  P(c)
        counts the hits at c or an ancestor of c; `call` is the lowest common ancestor of the hit targets with the largest
        P (n_best of them, P = p_best): a pure function of the multiset of the read's hits, whatever their order.
        `confident` climbs from call under the rule as read_support's climbs from final; tally as there."""
        return self._calls_offsets("votes", bases, offsets, start, stop, min_hits, min_permille, tally)

    def read_votes_fastq(self, text, recs, min_hits=0, min_permille=0, tally=None):
        """The same for a block of FASTQ text with its line index (uint32[n, 4], as Sample.classify_fastq): a record that
        fails stop - start >= k has no window and no hit, and a tally counts it nowhere."""
        return self._calls_fastq("votes", [(text, recs)], min_hits, min_permille, tally)

    def votes_from_hits_device(self, d_hit_offsets, d_hits, d_n_kmers, n_reads, d_out, min_hits=0, min_permille=0, stream=0):
        """The vote kernels alone on a CSR resident in HBM (raw pointers, as kid_db_read_hits_device left it);
        asynchronous on `stream`: kid_db_votes_from_hits_device.  d_out: kid_vote[n_reads] (VOTE_DTYPE)."""
        self._from_hits_device("votes", d_hit_offsets, d_hits, d_n_kmers, n_reads, d_out, min_hits, min_permille, stream)

    def read_votes_time(self):
        """-> (device ms, calls, reads) of the vote kernels alone since the last query"""
        return self._time(self._lib.kid_db_read_votes_time)

    def read_fragments(self, bases, offsets, start=None, stop=None, min_hits=0, min_permille=0, tally=None):
        """Call mate pairs as one fragment (kid_db_read_fragments): -> a structured array (FRAGMENT_DTYPE: final, confident,
        n_kmers, n_hits, s_final, s_confident, final_1, final_2), one record per fragment.  The batch holds 2 F reads in
        interleaved order: read 2i is mate 1 of fragment i, and read 2i + 1 is its mate 2.  The fragment's hit sequence
        is a_1 .. a_p, b_1 .. b_q: mate 1 first, m = p + q and n = n_1 + n_2.  final, confident, n_kmers, n_hits, s_final
        and s_confident are exactly the read_support record applied to that sequence with that n, under (min_hits,
        min_permille).  final_1 is the left fold of a_1 .. a_p alone, and final_2 that of b_1 .. b_q alone; each is 0
        without a hit.  msca is not associative, so final is not msca(final_1, final_2) in general.
        tally: a Sample of this database.  A counted fragment adds 1 to gcount[confident]: once per fragment, under 0
        when confident = 0.  When confident > 0, the fragment sets the seen bit of every hit of both mates with
        target > 1 (and under KID_OPT_ENTRY_DEPTH adds 1 to depth[entry] per such hit)."""
        return self._calls_offsets("fragments", bases, offsets, start, stop, min_hits, min_permille, tally)

    def read_fragments_fastq(self, text1, recs1, text2, recs2, min_hits=0, min_permille=0, tally=None):
        """The same for two blocks of FASTQ text with their line indexes (uint32[n, 4] each, as Sample.classify_fastq):
        record i of recs1 is mate 1 and record i of recs2 is mate 2.  A record with seq_len = 0 and qual_len = 0 is an
        absent mate.  A fragment is counted when at least one of its mates is kept by process_qual; a dropped mate
        contributes no hit and no window."""
        return self._calls_fastq("fragments", [(text1, recs1), (text2, recs2)], min_hits, min_permille, tally)

    def fragments_from_hits_device(self, d_hit_offsets, d_hits, d_n_kmers, n_reads, d_out, min_hits=0, min_permille=0, stream=0):
        """The fragment kernel alone on an interleaved CSR of n_reads = 2 F reads resident in HBM (raw pointers, as
        kid_db_read_hits_device left it); asynchronous on `stream`: kid_db_fragments_from_hits_device.
        d_out: kid_fragment[n_reads / 2] (FRAGMENT_DTYPE)."""
        self._from_hits_device("fragments", d_hit_offsets, d_hits, d_n_kmers, n_reads, d_out, min_hits, min_permille, stream)

    def read_fragments_time(self):
        """-> (device ms, calls, fragments) of the fragment kernel alone since the last query"""
        return self._time(self._lib.kid_db_read_fragments_time)

    def read_fragment_votes(self, bases, offsets, start=None, stop=None, min_hits=0, min_permille=0, tally=None):
        """Call mate pairs by root-path votes (kid_db_read_fragment_votes): -> a structured array (FRAGMENT_VOTE_DTYPE:
        call, confident, n_kmers, n_hits, p_best, n_best, s_call, s_confident, call_1, call_2), one record per fragment.
        The batch holds 2 F reads in interleaved order, as for read_fragments.  The first eight fields are exactly the
        read_votes record of a read with the hits of both mates (m = p + q) and n = n_1 + n_2 windows, under (min_hits,
        min_permille): a pure function of the two mates' hit multisets.  call_1 is the vote call of mate 1's hits alone
        and call_2 that of mate 2's; each is 0 without a hit.  Exchanging the mates exchanges call_1 and call_2 and
        changes nothing else.
        tally: a Sample of this database, counted exactly as read_fragments counts with this `confident`."""
        return self._calls_offsets("fragment_votes", bases, offsets, start, stop, min_hits, min_permille, tally)

    def read_fragment_votes_fastq(self, text1, recs1, text2, recs2, min_hits=0, min_permille=0, tally=None):
        """The same for two blocks of FASTQ text with their line indexes, as read_fragments_fastq: record i of recs1 is
        mate 1 and record i of recs2 is mate 2; a record with seq_len = 0 and qual_len = 0 is an absent mate.  A fragment
        is counted when at least one of its mates is kept by process_qual."""
        return self._calls_fastq("fragment_votes", [(text1, recs1), (text2, recs2)], min_hits, min_permille, tally)

    def fragment_votes_from_hits_device(self, d_hit_offsets, d_hits, d_n_kmers, n_reads, d_out, min_hits=0, min_permille=0, stream=0):
        """The fragment-vote kernels alone on an interleaved CSR of n_reads = 2 F reads resident in HBM (raw pointers, as
        kid_db_read_hits_device left it); asynchronous on `stream`: kid_db_fragment_votes_from_hits_device.
        d_out: kid_fragment_vote[n_reads / 2] (FRAGMENT_VOTE_DTYPE)."""
        self._from_hits_device("fragment_votes", d_hit_offsets, d_hits, d_n_kmers, n_reads, d_out, min_hits, min_permille, stream)

    def read_fragment_votes_time(self):
        """-> (device ms, calls, fragments) of the fragment-vote kernels alone since the last query"""
        return self._time(self._lib.kid_db_read_fragment_votes_time)

    def _read_segments(self, family, n, call):
        """the sizing call, then the call that fills a buffer of exactly that size: call(offsets, records, cap, total)"""
        offsets = np.empty(n + 1, np.uint64)
        total = C.c_uint64(0)
        check(call(_ptr(offsets), None, 0, C.byref(total)))
        records = np.zeros(total.value, _SEGMENT_FAMILIES[family])
        if total.value:
            check(call(_ptr(offsets), _ptr(records), total.value, C.byref(total)))
        return ReadSegments(offsets, records)

    def _segments_offsets(self, family, bases, offsets, start, stop, seg_len, seg_step, min_hits, min_permille):
        """kid_db_read_<family> over a batch held in host memory"""
        fn = getattr(self._lib, "kid_db_read_" + family)
        bases, offsets, start, stop, n = _offsets_batch(bases, offsets, start, stop)
        step = seg_len if seg_step is None else seg_step
        return self._read_segments(family, n, lambda o, s, cap, tot: fn(
            self._h, _ptr(bases), _ptr(offsets), _ptr(start), _ptr(stop), n, seg_len, step, min_hits, min_permille, o, s, cap, tot))

    def _segments_fastq(self, family, text, recs, seg_len, seg_step, min_hits, min_permille):
        """kid_db_read_<family>_fastq over a block of FASTQ text"""
        fn = getattr(self._lib, "kid_db_read_%s_fastq" % family)
        text, recs, n = _fastq_block(text, recs)
        step = seg_len if seg_step is None else seg_step
        return self._read_segments(family, n, lambda o, s, cap, tot: fn(
            self._h, _ptr(text), text.size, _ptr(recs), n, seg_len, step, min_hits, min_permille, o, s, cap, tot))

    def _segments_device(self, family, d_bases, bases_nbytes, d_offsets, n_reads, seg_len, seg_step, d_seg_offsets, d_n_hits, d_n_segments,
                         d_start, d_stop, min_hits, min_permille, d_hits, hits_cap, d_segments, seg_cap, stream):
        """kid_db_read_<family>_device: everything resident in HBM"""
        check(getattr(self._lib, "kid_db_read_%s_device" % family)(
            self._h, C.c_void_p(d_bases), bases_nbytes, C.c_void_p(d_offsets), C.c_void_p(d_start or None), C.c_void_p(d_stop or None),
            n_reads, seg_len, seg_len if seg_step is None else seg_step, min_hits, min_permille, C.c_void_p(d_hits or None), hits_cap,
            C.c_void_p(d_seg_offsets), C.c_void_p(d_segments or None), seg_cap, C.c_void_p(d_n_hits), C.c_void_p(d_n_segments),
            C.c_void_p(stream or None)))

    def read_segments(self, bases, offsets, start=None, stop=None, seg_len=1000, seg_step=None, min_hits=0, min_permille=0):
        """Call the records of a batch held in host memory in segments (kid_db_read_segments) -> ReadSegments.  A read
        with P window positions is cut into segments of seg_len positions, seg_step apart (None: seg_len; seg_len <=
        1024 * seg_step); each is called by its own hits under (min_hits, min_permille) as read_support calls a whole
        read.  `pos` is counted from the first byte of the read.  Pure: no sample is touched."""
        return self._segments_offsets("segments", bases, offsets, start, stop, seg_len, seg_step, min_hits, min_permille)

    def read_segments_fastq(self, text, recs, seg_len=1000, seg_step=None, min_hits=0, min_permille=0):
        """The same for a block of FASTQ text with its line index (uint32[n, 4], as Sample.classify_fastq): a record that
        fails stop - start >= k has no segment; KID_DB_OPT_MIN_BASE_QUALITY applies as in read_hits_fastq."""
        return self._segments_fastq("segments", text, recs, seg_len, seg_step, min_hits, min_permille)

    def read_segments_device(self, d_bases, bases_nbytes, d_offsets, n_reads, seg_len, seg_step, d_seg_offsets, d_n_hits, d_n_segments,
                             d_start=0, d_stop=0, min_hits=0, min_permille=0, d_hits=0, hits_cap=0, d_segments=0, seg_cap=0, stream=0):
        """Asynchronous, everything resident in HBM (raw pointers): kid_db_read_segments_device.  d_hits / hits_cap is the
        caller's scratch for the hits; no segment is written when the hits or the segments exceed their cap."""
        self._segments_device("segments", d_bases, bases_nbytes, d_offsets, n_reads, seg_len, seg_step, d_seg_offsets, d_n_hits, d_n_segments,
                              d_start, d_stop, min_hits, min_permille, d_hits, hits_cap, d_segments, seg_cap, stream)

    def read_segments_time(self):
        """-> (device ms, calls, reads) of the segment kernels alone since the last query"""
        return self._time(self._lib.kid_db_read_segments_time)

    def read_segment_votes(self, bases, offsets, start=None, stop=None, seg_len=1000, seg_step=None, min_hits=0, min_permille=0):
        """Call the records of a batch held in host memory in segments by root-path votes (kid_db_read_segment_votes)
        -> ReadSegments over SEGMENT_VOTE_DTYPE.  The segments are those of read_segments; each is called by the vote
        rule of read_votes over its own hits, so the call does not depend on their order (nor on the strand the record
        was assembled on).  Pure: no sample is touched."""
        return self._segments_offsets("segment_votes", bases, offsets, start, stop, seg_len, seg_step, min_hits, min_permille)

    def read_segment_votes_fastq(self, text, recs, seg_len=1000, seg_step=None, min_hits=0, min_permille=0):
        """The same for a block of FASTQ text with its line index, as read_segments_fastq (a dropped record has no segment;
        KID_DB_OPT_MIN_BASE_QUALITY and KID_DB_OPT_LOW_COMPLEXITY apply as there)."""
        return self._segments_fastq("segment_votes", text, recs, seg_len, seg_step, min_hits, min_permille)

    def read_segment_votes_device(self, d_bases, bases_nbytes, d_offsets, n_reads, seg_len, seg_step, d_seg_offsets, d_n_hits, d_n_segments,
                                  d_start=0, d_stop=0, min_hits=0, min_permille=0, d_hits=0, hits_cap=0, d_segments=0, seg_cap=0, stream=0):
        """Asynchronous, everything resident in HBM (raw pointers): kid_db_read_segment_votes_device, argument for argument
        read_segments_device with kid_segment_vote[seg_cap] (SEGMENT_VOTE_DTYPE) at d_segments."""
        self._segments_device("segment_votes", d_bases, bases_nbytes, d_offsets, n_reads, seg_len, seg_step, d_seg_offsets, d_n_hits, d_n_segments,
                              d_start, d_stop, min_hits, min_permille, d_hits, hits_cap, d_segments, seg_cap, stream)

    def read_segment_votes_time(self):
        """-> (device ms, calls, reads) of the segment scans and segment-vote kernels alone since the last query"""
        return self._time(self._lib.kid_db_read_segment_votes_time)

    def set_sites(self, org, pos):
        """Give the database its sites (kid_db_set_sites): org and pos hold fields 3 and 4 of the probe line of every entry,
        in the order the builder got them (what read_probe_sites yields); org < 2^24, pos < 2^31.  A second call replaces
        them; a replica starts without."""
        org = _as(org, np.uint32)
        pos = _as(pos, np.uint32)
        if org.shape != pos.shape or org.ndim != 1:
            raise ValueError("org and pos must be 1-D arrays of equal length")
        check(self._lib.kid_db_set_sites(self._h, _ptr(org), _ptr(pos), org.size))

    def clear_sites(self):
        """Free the sites: every read_loci call is KID_ERR_STATE until set_sites."""
        check(self._lib.kid_db_set_sites(self._h, None, None, 0))

    def _loci_offsets(self, family, bases, offsets, start, stop, params):
        """kid_db_read_<family> over a batch held in host memory -> its records, one per unit"""
        dtype, unit = _LOCI_FAMILIES[family]
        bases, offsets, start, stop, n = _offsets_batch(bases, offsets, start, stop)
        out = np.zeros(n // unit, dtype)
        check(getattr(self._lib, "kid_db_read_" + family)(self._h, _ptr(bases), _ptr(offsets), _ptr(start), _ptr(stop), n, *params, _ptr(out)))
        return out

    def _loci_fastq(self, family, blocks, params):
        """kid_db_read_<family>_fastq over one block (text, recs) of FASTQ text, or two: the mates -> one record per unit"""
        blocks = [_fastq_block(text, recs) for text, recs in blocks]
        n = blocks[0][2]
        if any(b[2] != n for b in blocks):
            raise ValueError("recs1 and recs2 must hold one record per fragment each")
        out = np.zeros(n, _LOCI_FAMILIES[family][0])
        texts = [a for text, recs, _ in blocks for a in (_ptr(text), text.size, _ptr(recs))]
        check(getattr(self._lib, "kid_db_read_%s_fastq" % family)(self._h, *texts, n, *params, _ptr(out)))
        return out

    def _loci_from_hits_device(self, family, d_hit_offsets, d_hits, d_n_kmers, n_reads, d_out, params, stream):
        """kid_db_<family>_from_hits_device: a family's kernels alone on a CSR resident in HBM"""
        check(getattr(self._lib, "kid_db_%s_from_hits_device" % family)(
            self._h, C.c_void_p(d_hit_offsets), C.c_void_p(d_hits or None), C.c_void_p(d_n_kmers), n_reads, *params, C.c_void_p(d_out),
            C.c_void_p(stream or None)))

    def read_loci(self, bases, offsets, start=None, stop=None, diag_bin=1):
        """Place the reads of a batch held in host memory by colinear hits (kid_db_read_loci): -> a structured array
        (LOCUS_DTYPE: org, strand, n_chain, n_org, n_other, n_hits, n_kmers, pos_first, pos_last, entry_first), one record
        per read.  A hit at read position r on entry e has the forward key (org[e], 0, floor((pos[e] - r) / diag_bin)) and
        the reverse key (org[e], 1, (pos[e] + r) / diag_bin); the chain is the set of hits with the most common key
        (ties: strand 0, then the lowest org, then the lowest diagonal), n_other the most common key's count on another
        org.  The chain lies at genome coordinate pos[entry_first] at read position pos_first."""
        return self._loci_offsets("loci", bases, offsets, start, stop, (diag_bin,))

    def read_loci_fastq(self, text, recs, diag_bin=1):
        """The same for a block of FASTQ text with its line index (uint32[n, 4], as Sample.classify_fastq): a record that
        fails stop - start >= k has no window and no hit; KID_DB_OPT_MIN_BASE_QUALITY and KID_DB_OPT_LOW_COMPLEXITY apply
        as in read_hits_fastq."""
        return self._loci_fastq("loci", [(text, recs)], (diag_bin,))

    def loci_from_hits_device(self, d_hit_offsets, d_hits, d_n_kmers, n_reads, d_out, diag_bin=1, stream=0):
        """The loci kernels alone on a CSR resident in HBM (raw pointers, as kid_db_read_hits_device left it); asynchronous
        on `stream`: kid_db_loci_from_hits_device.  d_out: kid_locus[n_reads] (LOCUS_DTYPE)."""
        self._loci_from_hits_device("loci", d_hit_offsets, d_hits, d_n_kmers, n_reads, d_out, (diag_bin,), stream)

    def read_loci_time(self):
        """-> (device ms, calls, reads) of the loci kernels alone since the last query"""
        return self._time(self._lib.kid_db_read_loci_time)

    def read_fragment_loci(self, bases, offsets, start=None, stop=None, diag_bin=1, max_span=1000):
        """Place mate pairs as one fragment by colinear hits (kid_db_read_fragment_loci): -> a structured array
        (FRAGMENT_LOCUS_DTYPE: org, orient, mates, n_chain, n_chain_1, n_chain_2, n_org, n_other, n_hits, n_kmers, lo, hi,
        pos_first_1, pos_last_1, pos_first_2, pos_last_2), one record per fragment.  The batch holds 2 F reads in interleaved
        order, as for read_fragments.  A paired placement takes a forward key (g, D) of one mate and a reverse key (g, E) of
        the other with D <= E and (E - D) * diag_bin <= max_span, and scores the sum of their counts; a solo placement is one
        key of one mate.  The best placement has the highest score (ties: paired first, then the keys' order); mates is 3
        for a paired best, 1 or 2 for a solo best, 0 without a hit; orient = 0 means mate 1 reads forward; [lo, hi] is the
        genome interval the chosen chains cover, the unsequenced middle of a paired best included."""
        return self._loci_offsets("fragment_loci", bases, offsets, start, stop, (diag_bin, max_span))

    def read_fragment_loci_fastq(self, text1, recs1, text2, recs2, diag_bin=1, max_span=1000):
        """The same for two blocks of FASTQ text with their line indexes, as read_fragments_fastq: record i of recs1 is mate
        1 and record i of recs2 is mate 2; a record with seq_len = 0 and qual_len = 0 is an absent mate.
        KID_DB_OPT_MIN_BASE_QUALITY and KID_DB_OPT_LOW_COMPLEXITY apply as in read_fragments_fastq."""
        return self._loci_fastq("fragment_loci", [(text1, recs1), (text2, recs2)], (diag_bin, max_span))

    def fragment_loci_from_hits_device(self, d_hit_offsets, d_hits, d_n_kmers, n_reads, d_out, diag_bin=1, max_span=1000, stream=0):
        """The fragment-loci kernels alone on an interleaved CSR of n_reads = 2 F reads resident in HBM (raw pointers);
        asynchronous on `stream`: kid_db_fragment_loci_from_hits_device.  d_out: kid_fragment_locus[n_reads / 2]
        (FRAGMENT_LOCUS_DTYPE)."""
        self._loci_from_hits_device("fragment_loci", d_hit_offsets, d_hits, d_n_kmers, n_reads, d_out, (diag_bin, max_span), stream)

    def read_fragment_loci_time(self):
        """-> (device ms, calls, fragments) of the fragment-loci kernels alone since the last query"""
        return self._time(self._lib.kid_db_read_fragment_loci_time)

    def pileup(self, bin_width=1000):
        """A pileup of placed reads per genome bin over this database's sites (kid_pileup_create): -> Pileup.  The
        database must outlive it."""
        return Pileup(self, bin_width)

    def shared_kmers(self, items):
        """K-mers shared between samples (kid_db_shared_kmers) -> int64[n, n, ntar]: [i, j, t] = the database entries of
        target t that items i and j both have a bit for; the diagonal is an item's own bits per target (a sample's
        ucount).  An item is a Sample (of this database or of a replica: its bitmap is exported to the host first) or a
        uint8 array of seen_bytes bytes in the layout of Sample.seen_export.  No sample changes."""
        info = self.info
        nbytes = max((info.n_entries + 127) // 128, 1) * 16
        return _shared_kmers(items, nbytes, info.ntar,
                             lambda ptrs, n, out: self._lib.kid_db_shared_kmers(self._h, ptrs, n, 0, _ptr(out)))

    def seen_coverage(self, items, org, pos, bin_width=1000):
        """Breadth of coverage per organism (kid_seen_coverage) on this database's device -> COVERAGE_DTYPE[n, n_orgs].  An
        item is a Sample (its bitmap is exported to the host first) or a uint8 array of seen_bytes bytes; org and pos hold
        fields 3 and 4 of the probe line of every entry of the database, in the order the builder got them."""
        info = self.info
        if np.size(org) != info.n_entries:
            raise ValueError("org has %d entries, the database has %d" % (np.size(org), info.n_entries))
        return seen_coverage(org, pos, items, bin_width=bin_width, device=info.device)

    def gather_ceiling(self, n_loads=1 << 28, inflight=4, iters=3):
        """Random gather rate over this DB's table: (ms per launch, loads per launch).  inflight 101 / 108: random
        128-byte lines asked for the way the classify kernel asks (64 per load / runs of 8 lanes), 4 loads in flight;
        1, 2, 4, 8: the round-1 cell probe (see include/kmer_id_amd.h)."""
        ms = C.c_float(0)
        loads = C.c_uint64(0)
        check(self._lib.kid_bench_gather(self._h, n_loads, inflight, iters, C.byref(ms), C.byref(loads)))
        return ms.value, loads.value

    def table_and_digest(self):
        """-> (table, digest) downloaded: uint32 [cells, 4] and uint32 [lines, 2] (None for a table without a digest
        plane).  For tests and tools: a full-size table is 16 GiB."""
        tp, dp, tb, db_ = C.c_void_p(), C.c_void_p(), C.c_uint64(0), C.c_uint64(0)
        check(self._lib.kid_bench_db_arrays(self._h, C.byref(tp), C.byref(tb), C.byref(dp), C.byref(db_)))
        dev = self.info.device
        table = np.empty((tb.value // 16, 4), np.uint32)
        check(self._lib.kid_dev_download(dev, _ptr(table), tp, tb.value))
        digest = None
        if dp.value:
            digest = np.empty((db_.value // 8, 2), np.uint32)
            check(self._lib.kid_dev_download(dev, _ptr(digest), dp, db_.value))
        return table, digest

    def sample(self):
        return Sample(self)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.kid_db_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Pileup:
    """Placed reads piled up per genome bin (kid_pileup_*): two uint32 counters per bin of bin_width bases, `starts` and
    `depth`, in the geometry of seen_coverage for the same bin width.  add() takes LOCUS_DTYPE records as read_loci
    returns them; a record is placed when n_chain >= min_chain, n_chain - n_other (0 when negative) >= min_margin, strand
    <= 1, entry_first < n_entries and org == org[entry_first].  With a = pos[entry_first], d = max(pos_last - pos_first, 0):
    forward lo = a, hi = a + d + k - 1; reverse lo = max(0, a - d), hi = a + k - 1; b_lo and b_hi are lo / W and hi / W
    clamped to span_bins - 1; the record adds 1 to starts[b_lo] and 1 to depth[b] for b in b_lo..b_hi.  The result does not
    depend on the order of the records, the split into calls or the stream.  A context manager; the database must outlive it."""

    def __init__(self, db, bin_width=1000):
        self._lib = db._lib
        self._h = None
        h = C.c_void_p()
        check(self._lib.kid_pileup_create(db._h, bin_width, C.byref(h)))
        self._h = h
        n_orgs, n_bins, w = C.c_uint32(0), C.c_uint64(0), C.c_uint32(0)
        check(self._lib.kid_pileup_info(self._h, C.byref(n_orgs), C.byref(n_bins), C.byref(w)))
        self.n_orgs, self.n_bins, self.bin_width = n_orgs.value, n_bins.value, w.value

    def add(self, loci, min_chain=2, min_margin=1):
        """Add LOCUS_DTYPE records held in host memory (kid_pileup_add)."""
        loci = np.ascontiguousarray(loci, LOCUS_DTYPE)
        check(self._lib.kid_pileup_add(self._h, _ptr(loci), loci.size, min_chain, min_margin))

    def add_device(self, ptr, n, min_chain=2, min_margin=1, stream=0):
        """Add n kid_locus records resident in HBM (a raw pointer); asynchronous on `stream`: kid_pileup_add_device."""
        check(self._lib.kid_pileup_add_device(self._h, C.c_void_p(ptr or None), n, min_chain, min_margin, C.c_void_p(stream or None)))

    def add_fragments(self, recs, min_chain=2, min_margin=1, paired_only=False):
        """Add FRAGMENT_LOCUS_DTYPE records held in host memory (kid_pileup_add_fragments): a record is placed over the
        bins of its own [lo, hi] on its org when mates is in 1..3 (3 alone under paired_only), n_chain >= min_chain, n_chain
        - n_other (0 when negative) >= min_margin, the org has a bin and lo <= hi.  Fragment and read records may share a
        pileup."""
        recs = np.ascontiguousarray(recs, FRAGMENT_LOCUS_DTYPE)
        check(self._lib.kid_pileup_add_fragments(self._h, _ptr(recs), recs.size, min_chain, min_margin, int(bool(paired_only))))

    def add_fragments_device(self, ptr, n, min_chain=2, min_margin=1, paired_only=False, stream=0):
        """Add n kid_fragment_locus records resident in HBM (a raw pointer); asynchronous on `stream`:
        kid_pileup_add_fragments_device."""
        check(self._lib.kid_pileup_add_fragments_device(self._h, C.c_void_p(ptr or None), n, min_chain, min_margin, int(bool(paired_only)),
                                                        C.c_void_p(stream or None)))

    def counts(self):
        """-> (records handed in, records placed)"""
        a, b = C.c_uint64(0), C.c_uint64(0)
        check(self._lib.kid_pileup_counts(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def summary(self):
        """-> PILEUP_DTYPE[n_orgs]: n_placed, span_bins, bins_covered, max_gap, max_depth, max_depth_bin, max_starts,
        max_starts_bin, reserved, depth_sum"""
        out = np.zeros(self.n_orgs, PILEUP_DTYPE)
        check(self._lib.kid_pileup_summary(self._h, _ptr(out)))
        return out

    def bins(self):
        """-> (bin_base uint64[n_orgs + 1], starts uint32[B], depth uint32[B]): organism g's bins lie at bin_base[g]"""
        base = np.zeros(self.n_orgs + 1, np.uint64)
        starts, depth = np.zeros(self.n_bins, np.uint32), np.zeros(self.n_bins, np.uint32)
        check(self._lib.kid_pileup_bins(self._h, _ptr(base), _ptr(starts), _ptr(depth), self.n_bins))
        return base, starts, depth

    def export(self):
        """-> (starts uint32[B], steps uint32[B + n_orgs]): what merge() of another pileup of the same geometry takes"""
        starts, steps = np.zeros(self.n_bins, np.uint32), np.zeros(self.n_bins + self.n_orgs, np.uint32)
        check(self._lib.kid_pileup_export(self._h, _ptr(starts), _ptr(steps)))
        return starts, steps

    def merge(self, starts, steps, n_records, n_placed):
        """Add the export of another pileup of the same geometry, element-wise with wrap-around (kid_pileup_merge)."""
        starts, steps = _as(starts, np.uint32), _as(steps, np.uint32)
        if starts.shape != (self.n_bins,) or steps.shape != (self.n_bins + self.n_orgs,):
            raise ValueError("starts and steps must have %d and %d elements" % (self.n_bins, self.n_bins + self.n_orgs))
        check(self._lib.kid_pileup_merge(self._h, _ptr(starts), _ptr(steps), n_records, n_placed))

    def reset(self):
        check(self._lib.kid_pileup_reset(self._h))

    def time(self):
        """-> (device ms, calls, records) of the add kernels alone since the last query"""
        ms, calls, records = C.c_double(0), C.c_uint64(0), C.c_uint64(0)
        check(self._lib.kid_pileup_time(self._h, C.byref(ms), C.byref(calls), C.byref(records)))
        return ms.value, calls.value, records.value

    def close(self):
        if getattr(self, "_h", None):
            self._lib.kid_pileup_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _shared_kmers(items, nbytes, ntar, call):
    """the items of a shared_kmers call as host bitmaps of nbytes bytes -> int64[n, n, ntar] from call(ptrs, n, out)"""
    maps = []
    for it in items:
        a = it.seen_export(0, it.seen_bytes()) if isinstance(it, Sample) else np.ascontiguousarray(it, np.uint8).reshape(-1)
        if a.size != nbytes:
            raise ValueError("a bitmap of %d bytes where the database's have %d" % (a.size, nbytes))
        maps.append(a)
    n = len(maps)
    ptrs = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in maps])
    out = np.zeros((n, n, ntar), np.int64)
    check(call(ptrs, n, out))
    return out


def shared_kmers(targets, ntar, bitmaps, device=0):
    """K-mers shared between samples without a database (kid_shared_kmers): targets[n_entries] as handed to the builder,
    bitmaps of ((n_entries + 127) // 128) * 16 bytes each (16 for no entries) -> int64[n, n, ntar] as KmerDB.shared_kmers."""
    lib = _lib.load()
    targets = _as(targets, np.uint32)
    nbytes = max((targets.size + 127) // 128, 1) * 16
    return _shared_kmers(bitmaps, nbytes, ntar,
                         lambda ptrs, n, out: lib.kid_shared_kmers(device, _ptr(targets), targets.size, ntar, ptrs, n, 0, _ptr(out)))


def shared_kmers_time():
    """-> (device ms, calls) of the kernels of the shared_kmers calls of this process since the last query"""
    ms, calls = C.c_double(0), C.c_uint64(0)
    check(_lib.load().kid_shared_kmers_time(C.byref(ms), C.byref(calls)))
    return ms.value, calls.value


# kid_coverage: one record per (bitmap, organism) (kid_seen_coverage)
COVERAGE_DTYPE = np.dtype([(name, np.uint32) for name in ("n_probes", "n_seen", "span_bins", "bins", "bins_seen", "max_gap",
                                                          "max_bin_seen", "max_bin")])


def _coverage_inputs(org, pos, bitmaps, n_orgs):
    """the arguments of a seen_coverage call -> (org, pos, n_orgs, the bitmaps as host arrays, their pointers)"""
    org, pos = _as(org, np.uint32).reshape(-1), _as(pos, np.uint32).reshape(-1)
    if org.size != pos.size:
        raise ValueError("org has %d entries, pos has %d" % (org.size, pos.size))
    if n_orgs is None:
        n_orgs = int(org.max()) + 1 if org.size else 0
    nbytes = max((org.size + 127) // 128, 1) * 16
    maps = []
    for it in bitmaps:
        a = it.seen_export(0, it.seen_bytes()) if isinstance(it, Sample) else np.ascontiguousarray(it, np.uint8).reshape(-1)
        if a.size != nbytes:
            raise ValueError("a bitmap of %d bytes where %d entries have %d" % (a.size, org.size, nbytes))
        maps.append(a)
    ptrs = (C.c_void_p * max(len(maps), 1))(*[a.ctypes.data for a in maps])
    return org, pos, n_orgs, maps, ptrs


def seen_coverage(org, pos, bitmaps, bin_width=1000, n_orgs=None, device=0):
    """Breadth of coverage per organism (kid_seen_coverage): org[n_entries] and pos[n_entries] are fields 3 and 4 of the
    probe line every entry came from, bitmaps of ((n_entries + 127) // 128) * 16 bytes each (16 for no entries) in the
    layout of Sample.seen_export -> COVERAGE_DTYPE[n, n_orgs].  n_orgs: the largest org + 1 unless given."""
    org, pos, n_orgs, maps, ptrs = _coverage_inputs(org, pos, bitmaps, n_orgs)
    out = np.zeros((len(maps), n_orgs), COVERAGE_DTYPE)
    check(_lib.load().kid_seen_coverage(device, _ptr(org), _ptr(pos), org.size, n_orgs, bin_width, ptrs, len(maps), _ptr(out)))
    return out


def seen_coverage_bins(org, pos, bitmaps, bin_width=1000, n_orgs=None, device=0):
    """The per-bin profile behind seen_coverage (kid_seen_coverage_bins) -> (bin_base uint64[n_orgs + 1], probes_per_bin
    uint32[B], seen_per_bin uint32[n, B]): the bins of organism g are bin_base[g] .. bin_base[g + 1] - 1."""
    lib = _lib.load()
    org, pos, n_orgs, maps, ptrs = _coverage_inputs(org, pos, bitmaps, n_orgs)
    base = np.zeros(n_orgs + 1, np.uint64)
    n_bins = C.c_uint64(0)
    check(lib.kid_seen_coverage_bins(device, _ptr(org), _ptr(pos), org.size, n_orgs, bin_width, ptrs, len(maps), _ptr(base), None, None, 0,
                                     C.byref(n_bins)))
    B = n_bins.value
    probes, seen = np.zeros(B, np.uint32), np.zeros((len(maps), B), np.uint32)
    check(lib.kid_seen_coverage_bins(device, _ptr(org), _ptr(pos), org.size, n_orgs, bin_width, ptrs, len(maps), _ptr(base), _ptr(probes),
                                     _ptr(seen), B, C.byref(n_bins)))
    return base, probes, seen


def seen_coverage_time():
    """-> (device ms, calls) of the kernels of the seen_coverage calls of this process since the last query"""
    ms, calls = C.c_double(0), C.c_uint64(0)
    check(_lib.load().kid_seen_coverage_time(C.byref(ms), C.byref(calls)))
    return ms.value, calls.value


def read_probe_sites(path, k=30):
    """(org, pos) as uint32 arrays, one pair per database entry in file order, from a probes file (plain or .gz) whose
    lines are SEQ,target,org,position,strand,count: a line gives its org and position to each of its entries, one per
    window of k upper-case ACGT bases.  Plain Python, for users without a front-end; a line that does not parse is
    skipped, as the loader of the front-ends skips it."""
    import gzip
    import re
    runs = re.compile(rb"[ACGT]+")
    org, pos = [], []
    with open(path, "rb") as f:
        gz = f.read(2) == b"\x1f\x8b"
    with (gzip.open(path, "rb") if gz else open(path, "rb")) as f:
        for line in f:
            if not line.endswith(b"\n"):
                break  # the unterminated last line is dropped
            fields = line.replace(b",", b" ").split()
            if len(fields) < 6:
                continue
            try:
                int(fields[1]), int(fields[5])
                o, p = int(fields[2]), int(fields[3])
            except ValueError:
                continue
            n = sum(max(len(r) - k + 1, 0) for r in runs.findall(fields[0]))
            if n == 0:
                continue
            if o < 0 or p < 0:
                raise ValueError("%s: org or position outside 0..2^32-1 in %r" % (path, line[:120]))
            if o >= 1 << 31 or p >= 1 << 31:
                continue  # (the loader reads both as int: such a line fails to parse and gives no entry to any front-end)
            org.append(np.full(n, o, np.uint32))
            pos.append(np.full(n, p, np.uint32))
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, np.uint32)  # noqa: E731
    return cat(org), cat(pos)


SEEN_MAGIC = b"KIDSEEN1"


def write_seen_file(path, bitmap, n_entries, ntar, k):
    """A seen file (what --seen writes beside a result file): a 32-byte little-endian header -- the 8 bytes KIDSEEN1, uint64
    n_entries, int32 ntar, int32 k, uint64 nbytes -- and nbytes bytes of bitmap."""
    bitmap = np.ascontiguousarray(bitmap, np.uint8).reshape(-1)
    with open(path, "wb") as f:
        f.write(SEEN_MAGIC + struct.pack("<QiiQ", n_entries, ntar, k, bitmap.size))
        f.write(bitmap.tobytes())


def read_seen_file(path):
    """-> (bitmap uint8[nbytes], n_entries, ntar, k) of a seen file; ValueError for a bad magic, a size that does not fit
    n_entries, or a truncated file."""
    with open(path, "rb") as f:
        head = f.read(32)
        if len(head) < 32 or head[:8] != SEEN_MAGIC:
            raise ValueError("%s is not a seen file (bad magic)" % path)
        n_entries, ntar, k, nbytes = struct.unpack("<QiiQ", head[8:])
        if nbytes != max((n_entries + 127) // 128, 1) * 16:
            raise ValueError("%s: %d bytes of bitmap do not fit %d entries" % (path, nbytes, n_entries))
        data = f.read(nbytes + 1)
    if len(data) != nbytes:
        raise ValueError("%s is truncated or has bytes behind its bitmap" % path)
    return np.frombuffer(data, np.uint8).copy(), n_entries, ntar, k


def end_merged(samples):
    """One sample of the input dealt out over several Sample objects (one per GPU / replica) -> (gcount, ucount)."""
    lib = _lib.load()
    n = len(samples)
    arr = (C.c_void_p * n)(*[s._h for s in samples])
    ntar = samples[0].ntar
    g = np.empty(ntar, np.int64)
    u = np.empty(ntar, np.int64)
    check(lib.kid_sample_end_merged(arr, n, _ptr(g), _ptr(u)))
    return g, u


def depth_spectrum_merged(samples, bins=256):
    """The depth spectrum of one sample of the input dealt out over several Sample objects (one per GPU / replica), every
    one with KID_OPT_ENTRY_DEPTH on -> (spectrum[ntar, bins], ksum, dmax) of the summed counters; no sample changes."""
    lib = _lib.load()
    n = len(samples)
    arr = (C.c_void_p * n)(*[s._h for s in samples])
    ntar = samples[0].ntar
    spectrum, ksum, dmax = np.empty((ntar, bins), np.uint64), np.empty(ntar, np.uint64), np.empty(ntar, np.uint32)
    check(lib.kid_sample_depth_spectrum_merged(arr, n, bins, _ptr(spectrum), _ptr(ksum), _ptr(dmax)))
    return spectrum, ksum, dmax


class Sample:
    """Per-sample counters; replaces the reset at newkmer_10nx.cpp:1017-1019."""

    def __init__(self, db):
        self.db = db
        self._lib = db._lib
        h = C.c_void_p()
        check(self._lib.kid_sample_begin(db._h, C.byref(h)))
        self._h = h
        self.ntar = db.info.ntar

    def reset(self):
        check(self._lib.kid_sample_reset(self._h))

    def set_option(self, option, value=1):
        check(self._lib.kid_sample_set_option(self._h, option, value))

    def masked_bases(self):
        """-> bases masked under KID_OPT_MIN_BASE_QUALITY since the sample began or was last reset"""
        n = C.c_uint64(0)
        check(self._lib.kid_sample_masked_bases(self._h, C.byref(n)))
        return n.value

    def low_complexity_bases(self):
        """-> bases masked under KID_OPT_LOW_COMPLEXITY since the sample began or was last reset"""
        n = C.c_uint64(0)
        check(self._lib.kid_sample_lowc_bases(self._h, C.byref(n)))
        return n.value

    def classify(self, bases, offsets, start=None, stop=None, want_final=True):
        """process_read for a batch held in host memory; returns final_targ per read."""
        bases, offsets, start, stop, n = _offsets_batch(bases, offsets, start, stop)
        out = np.empty(n, np.uint32) if want_final else None
        check(self._lib.kid_classify_batch(self._h, _ptr(bases), _ptr(offsets), _ptr(start), _ptr(stop), n, _ptr(out)))
        return out

    @staticmethod
    def _borrowed(a, dtype, name):
        """an array the library reads / writes in place until wait(): it must already be what the C ABI expects"""
        if a is None:
            return None
        if not isinstance(a, np.ndarray) or a.dtype != np.dtype(dtype) or not a.flags["C_CONTIGUOUS"]:
            raise TypeError("%s must be a C-contiguous numpy array of %s (it is handed to the library as it is, not copied)" % (name, np.dtype(dtype)))
        return a

    def classify_async(self, bases, offsets, start=None, stop=None, out=None):
        """Queue a batch held in host memory (numpy arrays or PinnedBuffer views, which the caller keeps alive and
        untouched until wait(ticket)); -> ticket.  `out`: uint32[n] array that receives final_targ (or None)."""
        bases = self._borrowed(bases, np.uint8, "bases")
        offsets = self._borrowed(offsets, np.uint64, "offsets")
        start = self._borrowed(start, np.int32, "start")
        stop = self._borrowed(stop, np.int32, "stop")
        out = self._borrowed(out, np.uint32, "out")
        n = offsets.size - 1
        if out is not None and out.size < n:
            raise ValueError("out holds fewer than %d entries" % n)
        t = C.c_uint64(0)
        check(self._lib.kid_classify_batch_async(self._h, _ptr(bases), _ptr(offsets), _ptr(start), _ptr(stop), n, _ptr(out), C.byref(t)))
        return t.value

    def classify_fastq(self, text, recs):
        """A block of FASTQ text with its line index (uint32[n, 4]: seq_off, seq_len, qual_off, qual_len): process_qual,
        the >= k test and process_read on the GPU (kid_classify_fastq_async).  -> (final_targ, start, stop)"""
        text, recs, n = _fastq_block(text, recs)
        final = np.empty(n, np.uint32)
        start = np.empty(n, np.int32)
        stop = np.empty(n, np.int32)
        t = C.c_uint64(0)
        check(self._lib.kid_classify_fastq_async(self._h, _ptr(text), text.size, _ptr(recs), n, _ptr(final), _ptr(start), _ptr(stop), C.byref(t)))
        self.wait(t.value)
        return final, start, stop

    def classify_fixed_async(self, bases_ptr, read_len, n_reads, out_ptr=0):
        """fixed-length whole reads back to back at the raw host address bases_ptr; -> ticket"""
        t = C.c_uint64(0)
        check(self._lib.kid_classify_fixed_async(self._h, C.c_void_p(bases_ptr), read_len, n_reads, C.c_void_p(out_ptr or None), C.byref(t)))
        return t.value

    def wait(self, ticket):
        check(self._lib.kid_classify_wait(self._h, ticket))

    def classify_device(self, d_bases, bases_nbytes, d_offsets, n_reads, d_start=0, d_stop=0, d_out=0, stream=0):
        """Asynchronous, device-resident inputs (raw pointers)."""
        check(self._lib.kid_classify_batch_device(self._h, C.c_void_p(d_bases), bases_nbytes, C.c_void_p(d_offsets),
                                                  C.c_void_p(d_start or None), C.c_void_p(d_stop or None), n_reads,
                                                  C.c_void_p(d_out or None), C.c_void_p(stream or None)))

    def classify_fixed_device(self, d_bases, read_len, n_reads, d_out=0, stream=0):
        check(self._lib.kid_classify_fixed_device(self._h, C.c_void_p(d_bases), read_len, n_reads,
                                                  C.c_void_p(d_out or None), C.c_void_p(stream or None)))

    def end(self):
        """-> (gcount[ntar], ucount[ntar]) as written to <prefix>_result.txt."""
        g = np.empty(self.ntar, np.int64)
        u = np.empty(self.ntar, np.int64)
        check(self._lib.kid_sample_end(self._h, _ptr(g), _ptr(u)))
        return g, u

    def gcount(self):
        g = np.empty(self.ntar, np.int64)
        check(self._lib.kid_sample_gcount(self._h, _ptr(g)))
        return g

    def ucount_range(self, slot_begin, slot_end):
        u = np.empty(self.ntar, np.int64)
        check(self._lib.kid_sample_ucount_range(self._h, slot_begin, slot_end, _ptr(u)))
        return u

    def stats(self):
        out = np.zeros(4, np.uint64)
        check(self._lib.kid_sample_stats(self._h, _ptr(out)))
        return {"reads": int(out[0]), "lookups": int(out[1]), "probes": int(out[2]), "hits": int(out[3])}

    def set_timing(self, enabled=True):
        check(self._lib.kid_sample_set_timing(self._h, 1 if enabled else 0))

    def kernel_time(self):
        """-> (total ms, launches) of kid_classify_kernel since the last call (HIP events on the launch stream)"""
        ms, n = C.c_double(0), C.c_uint64(0)
        check(self._lib.kid_sample_kernel_time(self._h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def kernel_times(self, cap=None):
        """-> (ms float64[min(cap, n)], n): the HIP-event time of each timed batch since the last call of this method,
        oldest first (kid_sample_kernel_times); cap=None asks for all of them"""
        n = C.c_uint64(0)
        if cap is None:
            cap = 1 << 16  # (as many as a sample keeps)
        ms = np.empty(cap, np.float64)
        check(self._lib.kid_sample_kernel_times(self._h, ms.ctypes.data_as(C.POINTER(C.c_double)), cap, C.byref(n)))
        return ms[:min(cap, n.value)], n.value

    def kernel_time_device(self):
        """-> (total ms, batches) of kid_classify_kernel since the last call, on the device's own 100 MHz clock"""
        ms, n = C.c_double(0), C.c_uint64(0)
        check(self._lib.kid_sample_kernel_time_device(self._h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def kernel_variants(self, digest=None):
        """-> the kid_classify_kernel instantiations launched since the sample began or was last reset, as a set of
        (ROWS, HIST, MINLOC, KFIX, PAIRK) tuples (kid_sample_kernel_variants).  digest=False: only those that read table
        headers; True: only the DIGEST instantiations of the pair and duo loops (KID_OPT_LINE_DIGEST); None: both."""
        m = C.c_uint64(0)
        check(self._lib.kid_sample_kernel_variants(self._h, C.byref(m)))
        hdr = {(b >> 3 & 1, b >> 2 & 1, b >> 1 & 1, 30 if b & 1 else 0, b >> 4) for b in range(48) if m.value >> b & 1}
        dig = {(b >> 2 & 1, b >> 1 & 1, 1, 30 if b & 1 else 0, 1 + (b >> 3)) for b in range(16) if m.value >> (48 + b) & 1}
        return hdr | dig if digest is None else dig if digest else hdr

    def log_state(self):
        """-> {"passes", "has_log", "logging"}: passes over the hit log queued since the sample began or was last reset,
        whether the sample has a log, and whether the device still logs (kid_sample_log_state).  Synchronises; applies
        nothing and changes nothing."""
        passes, has_log, logging = C.c_uint32(0), C.c_int(0), C.c_int(0)
        check(self._lib.kid_sample_log_state(self._h, C.byref(passes), C.byref(has_log), C.byref(logging)))
        return {"passes": passes.value, "has_log": bool(has_log.value), "logging": bool(logging.value)}

    def seen_bytes(self):
        n = C.c_uint64(0)
        check(self._lib.kid_sample_seen_bytes(self._h, C.byref(n)))
        return n.value

    def seen_export(self, byte_off, nbytes, dst_ptr=None, on_device=False):
        if dst_ptr is None:
            buf = np.empty(nbytes, np.uint8)
            check(self._lib.kid_sample_seen_export(self._h, byte_off, nbytes, _ptr(buf), 0))
            return buf
        check(self._lib.kid_sample_seen_export(self._h, byte_off, nbytes, C.c_void_p(dst_ptr), 1 if on_device else 0))
        return None  # dst_ptr may be a host pointer too (on_device=False)

    def seen_or(self, byte_off, src, nbytes=None, on_device=False):
        if isinstance(src, np.ndarray):
            src = np.ascontiguousarray(src, np.uint8)
            check(self._lib.kid_sample_seen_or(self._h, byte_off, src.size, _ptr(src), 0))
        else:
            check(self._lib.kid_sample_seen_or(self._h, byte_off, nbytes, C.c_void_p(src), 1 if on_device else 0))

    def depth_spectrum(self, bins=256):
        """Under KID_OPT_ENTRY_DEPTH -> (spectrum[ntar, bins], ksum[ntar], dmax[ntar]): per target, the number of its
        database entries hit b times (the last column: bins - 1 times or more; column 0: never), the sum of the counters
        and the largest (kid_sample_depth_spectrum)."""
        spectrum, ksum, dmax = np.empty((self.ntar, bins), np.uint64), np.empty(self.ntar, np.uint64), np.empty(self.ntar, np.uint32)
        check(self._lib.kid_sample_depth_spectrum(self._h, bins, _ptr(spectrum), _ptr(ksum), _ptr(dmax)))
        return spectrum, ksum, dmax

    def entry_depth(self, begin=0, end=None):
        """-> uint32[end - begin]: how often the tallies hit the database entries [begin, end) (end=None: the last entry)"""
        if end is None:
            end = self.db.info.n_entries
        out = np.empty(max(int(end) - int(begin), 0), np.uint32)
        check(self._lib.kid_sample_depth_export(self._h, begin, out.size, _ptr(out), 0))
        return out

    def depth_add(self, begin, array):
        """a saturating add of `array` (uint32) onto the counters of the entries from `begin` on (kid_sample_depth_add)"""
        array = _as(array, np.uint32)
        check(self._lib.kid_sample_depth_add(self._h, begin, array.size, _ptr(array), 0))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.kid_sample_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
