"""Inputs of tests/test_gpu_output_edges.py and tests/test_output_edge_cases.py: the smallest inputs that reach the paths of
the output half of the file pipeline -- traceback runs -> final CIGAR -> BAM records -> BGZF members -- which only open above
a wave size (64) or a share size (256 threads).  Every threshold stands next to the constant of the kernel source it
comes from.

  1. kernels.hpp WaveProbe: how far an indel run slides left through the match run in front of it, PROBE_ROUND positions
     per round.  slide_cases(): reads of one repeat between random flanks with one unit lost (D) or gained (I) at the
     repeat's right end; the chunks of a small max_b_rows keep align() from placing the indel further left than its
     chunk's first cell, and the standardisation moves it the rest of the way: up to 600 positions, ending on a base
     that differs (the flank, or a base that breaks the period in both sequences) or because the match run is used up
     (a foreign base inserted into the read inside the repeat).
  2. bam_deflate_kernels.hpp place_deflate_kernel: PLACE_THREADS threads share the batch's members, `seg` =
     ceil(n / 256) consecutive members each.  MEMBER_CASES: 257, 513 and 599 members.
  3. bam_emit_kernels.hpp wave_copy<NIB>: head bytes up to the first aligned word of the destination, words built from
     two aligned source words, tail bytes.  copy_records(): short reads as a product of name lengths, leading clips and
     lengths; copy_calls() states every wave_copy call of emit_bam_records_kernel for a batch of them.
"""
import numpy as np

# ---- 1. kernels.hpp WaveProbe --------------------------------------------------------------------------------------------
PROBE_ROUND = 64                             # kernels.hpp WaveProbe: positions compared per round (`if (n < 64) break;`)
SLIDE_TARGETS = tuple(k * PROBE_ROUND + d for k in (1, 2, 3) for d in (-1, 0, 1))      # 63 64 65 127 128 129 191 192 193
SLIDE_LONG = 4 * PROBE_ROUND + 1             # 257: a fifth round
SLIDE_CONTEXTS = [(30, 333), (30, 100), (10, 37)]            # (r, max_b_rows)
SLIDE_MAX_BASES = 700
UNIT8 = (1, 2, 3, 4, 1, 1, 2, 2)             # period 8 and no shorter one: above max_n = 6, the n-polymer states stay out
UNIT_FAMILIES = ((1,), (1, 2), (1, 2, 3))    # a homopolymer, periods 2 and 3: raw strings with blocks of I and D runs


def _other(rng, *avoid):
    return int(rng.choice([b for b in (1, 2, 3, 4) if b not in avoid]))


def slide_read(rng, unit, reps, fl, fr, kind, foreign_at=None, break_at=None):
    """-> ref, seq, cigar (op string).  flank(fl) + unit * reps + flank(fr) with one unit dropped from the read (kind 'D')
    or appended to it (kind 'I') at the repeat's right end; the flank bases next to the repeat end the period.
    break_at: the repeat base at that offset is another one in both sequences (it stays '=').  foreign_at: a base that
    differs from both neighbours is inserted into the read in front of the repeat base at that offset (one 'I')."""
    p = len(unit)
    left = [int(x) for x in rng.integers(1, 5, fl)]
    right = [int(x) for x in rng.integers(1, 5, fr)]
    if left:
        left[-1] = _other(rng, unit[-1], unit[0])
    if right:
        right[0] = _other(rng, unit[0], unit[-1])
    rep = list(unit) * reps
    if break_at is not None:
        rep[break_at] = _other(rng, rep[break_at], rep[break_at - 1], rep[(break_at + 1) % len(rep)])
    ref, seq, cig = left + rep, list(left), ["="] * fl
    body = rep[:len(rep) - p] if kind == "D" else rep
    for j, b in enumerate(body):
        if j == foreign_at:
            seq.append(_other(rng, body[j - 1], b))
            cig.append("I")
        seq.append(b)
        cig.append("=")
    if kind == "D":
        cig += ["D"] * p
    else:
        seq += list(unit)
        cig += ["I"] * p
    ref += right; seq += right; cig += ["="] * fr
    return np.array(ref, np.uint8), np.array(seq, np.uint8), "".join(cig)


def slide_cases(seed=64):
    """-> refs, seqs, cigs, labels.  Sweeps, each for D and for I (see SLIDE_SWEEPS for what each is for)."""
    rng = np.random.default_rng(seed)
    refs, seqs, cigs, labels = [], [], [], []

    def add(label, *a, **kw):
        r_, s_, c_ = slide_read(rng, *a, **kw)
        assert max(len(r_), len(s_)) <= SLIDE_MAX_BASES, (label, len(r_), len(s_))
        refs.append(r_); seqs.append(s_); cigs.append(c_); labels.append(label)

    for kind in "DI":
        for name, unit, reps, fl, fr, sweep in SLIDE_SWEEPS:
            for v in sweep:
                if name == "flank":
                    add((name, kind, v), unit, reps, v, fr, kind)
                elif name == "break":
                    add((name, kind, v), unit, reps, fl, fr, kind, break_at=v)
                elif name == "foreign":
                    add((name, kind, v), unit, reps, fl, fr, kind, foreign_at=v)
                else:
                    add((name, kind, len(unit), v), unit, v, fl, fr, kind)
    return refs, seqs, cigs, labels


# (name, unit, copies, left flank, right flank, the swept values).  At max_b_rows = 333 the chunk that holds the indel of these
# reads begins near row 333, and the indel cannot lie in front of it (raw strings like '332=8D40='):
#   flank    the left flank's length: the slide ends on the flank's last base
#   break    the offset of a base that breaks the period in both sequences: the slide ends on it
#   foreign  the offset of a base inserted into the read alone: the match run in front of the indel ends there
#   family   the number of copies of a shorter unit: n-polymer states, raw strings with blocks of I and D
SLIDE_SWEEPS = (
    ("flank", UNIT8, 40, None, 30, range(150, 300, 3)),
    ("break", UNIT8, 40, 30, 30, range(70, 300)),
    ("foreign", UNIT8, 40, 30, 30, (*range(16, 70, 6), *range(70, 300))),
    ("break", UNIT8, 80, 20, 20, range(330, 400, 8)),
    ("foreign", UNIT8, 80, 20, 20, range(330, 400, 8)),
    ("family", UNIT_FAMILIES[0], None, 30, 30, (90, 200, 350, 600)),
    ("family", UNIT_FAMILIES[1], None, 30, 30, (60, 120, 200, 300)),
    ("family", UNIT_FAMILIES[2], None, 30, 30, (40, 80, 130, 200)),
)


def glue_test_inputs(make_batch):
    """The reads of tests/test_gpu_parity.py::test_device_glue_equals_host_glue, drawn as that test draws them (it builds
    them inside its body) and its three (r, max_b_rows): none of their indel runs slides PROBE_ROUND positions, which
    tests/test_output_edge_cases.py asserts.  make_batch: npore_amd.synth.make_batch."""
    refs, seqs, cigs = make_batch(909, 24, ref_len=3000, p_np=0.2)
    r2, s2, c2 = make_batch(910, 40, ref_len=400, p_np=0.6)
    refs += r2; seqs += s2; cigs += c2
    rng = np.random.default_rng(5)
    for k in range(12):
        n = int(rng.integers(50, 400))
        ref = rng.integers(1, 3, size=n).astype(np.uint8)
        ops, seq, j = [], [], 0
        while j < n:
            e = rng.random()
            if e < 0.12:
                ops.append("D"); j += 1
            elif e < 0.24:
                ops.append("I"); seq.append(int(rng.integers(1, 3)))
            else:
                ops.append("="); seq.append(int(ref[j])); j += 1
        refs.append(ref); seqs.append(np.array(seq, np.uint8)); cigs.append("".join(ops))
    for k in range(3):
        ref, seq = refs[k], seqs[k]
        m = min(len(ref), len(seq)) - 40
        refs.append(ref); seqs.append(seq)
        cigs.append("I" * (len(seq) - m) + "D" * (len(ref) - m) + "=" * m)
    return refs, seqs, cigs, [(30, 20000), (100, 700), (10, 37)]


# ---- 2. bam_deflate_kernels.hpp place_deflate_kernel ---------------------------------------------------------------------
PLACE_THREADS = 256                          # place_deflate_kernel's one workgroup: `seg = (n + 255) / 256`
P = 65280                                    # DEFLATE_MEMBER_PAYLOAD: the bytes of a whole member
# (bytes, phase, whole members, seg, the first thread whose share is empty).  The third: a head fragment of P - 777 bytes
# leaves 599 whole members of the 600 P + 77 bytes, and thread 199 a share of two
MEMBER_CASES = [(257 * P + 1000, 0, 257, 2, 129), (513 * P + 1000, P - 3, 513, 3, 171), (600 * P + 77, 5 * P + 777, 599, 3, 200)]
PIPELINE_READS = 1200                        # reads of 10 kb in one batch: about 15 KB of record each


def place_shares(n):
    """(seg, [(k0, k1)] per thread) of place_deflate_kernel for n members"""
    seg = (n + PLACE_THREADS - 1) // PLACE_THREADS
    return seg, [(min(n, t * seg), min(n, min(n, t * seg) + seg)) for t in range(PLACE_THREADS)]


def member_cuts(n, phase):
    """(head fragment, whole members, tail fragment) of n bytes that begin at stream position `phase` (deflate_cuts)"""
    first = (P - phase % P) % P
    if n < first:
        return n, 0, 0
    return first, (n - first) // P, (n - first) % P


# ---- 3. bam_emit_kernels.hpp wave_copy ------------------------------------------------------------------------------------
COPY_LANES = 64                              # wave_copy: the word loop's stride (`w += 64`); n_words of 64 and 65 make its second trip
COPY_TAIL_LANE = 60                          # wave_copy: `lane >= 60` store the bytes behind the last whole word
NAME_LENGTHS = (1, 2, 3, 4)                  # l_read_name 2 ... 5: every residue mod 4
LEADS = (0, 1, 2, 3, 6, 7)                   # leading soft clips: both nibble parities, lead >> 1 in 0, 1, 3
SHORT_SL = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17)
LONG_SL = (511, 512, 513, 519, 520, 521)     # (sl + 1) / 2 = 256, 257, 260, 261: 64 and 65 words behind a head of 0 or 1
COPY_HPS = (None, 2, 256, 70000, -1, -129)   # no tag, and the widths 1, 2, 4, 1, 2
SEQ16 = "=ACMGRSVTWYHKDBN"
COPY_CONTIG = "ctg"


def copy_records(seed=60):
    """-> references, contig, records, pairs.  One read per (name length, lead, sl) of NAME_LENGTHS x LEADS x (SHORT_SL + LONG_SL);
    the trailing clip (0 / 1), the qualities (absent for a third), the HP tag and a hard clip in front cycle with sums of
    the three indices, so that none of them follows one axis.  '=' runs with one I of 2 and one D of 1 where sl >= 15.
    All on one contig, in coordinate order, 3 ... 9 bases apart.  pairs[k] = (ref, seq, op string) of read k without its
    clips: what align() is given."""
    rng = np.random.default_rng(seed)
    sls = SHORT_SL + LONG_SL
    contig, records, pairs = [], [], []
    for a, ln in enumerate(NAME_LENGTHS):
        for b, lead in enumerate(LEADS):
            for c, sl in enumerate(sls):
                k = len(records)
                contig += [int(x) for x in rng.integers(1, 5, 3 + (a + b + c) % 7)]
                pos = len(contig)
                trail, hard = (a + b + c) % 2, (a + 2 * b + c) % 5 == 1
                qual_absent = (a + b + 2 * c) % 3 == 0
                if sl >= 15:
                    m0 = sl // 3
                    m1 = (sl - 2 - m0) // 2
                    m2 = sl - 2 - m0 - m1
                    ref = [int(x) for x in rng.integers(1, 5, m0 + m1 + 1 + m2)]
                    ins = [int(x) for x in rng.integers(1, 5, 2)]
                    seq = ref[:m0] + ins + ref[m0:m0 + m1] + ref[m0 + m1 + 1:]
                    body = [(7, m0), (1, 2), (7, m1), (2, 1), (7, m2)]
                    ops = "=" * m0 + "II" + "=" * m1 + "D" + "=" * m2
                else:
                    ref = [int(x) for x in rng.integers(1, 5, sl)]
                    seq, body, ops = list(ref), [(7, sl)], "=" * sl
                assert len(seq) == sl
                contig += ref
                clip = lambda n: "".join(SEQ16[x] for x in rng.integers(1, 16, n))
                text = clip(lead) + "".join("NACGT"[x] for x in seq) + clip(trail)
                cigar = ([(5, 3)] if hard else []) + ([(4, lead)] if lead else []) + body + ([(4, trail)] if trail else [])
                name = "".join("abcdefghijklmnopqrstuvwxyz"[(k // 26 ** j) % 26] for j in range(ln))
                records.append(dict(name=name, flag=16 if k % 4 == 1 else 0, ref_id=0, pos=pos, mapq=k % 61, cigar=cigar, seq=text,
                                    qual=None if qual_absent else bytes(rng.integers(0, 60, len(text)).tolist()),
                                    hp=COPY_HPS[(a + b + c) % len(COPY_HPS)], _lead=lead, _trail=trail, _sl=sl))
                pairs.append((np.array(ref, np.uint8), np.array(seq, np.uint8), ops))
    contig += [int(x) for x in rng.integers(1, 5, 40)]
    contig = "".join("NACGT"[x] for x in contig)
    return [(COPY_CONTIG, len(contig))], contig, records, pairs


def _hp_bytes(hp):
    hp = hp or 0
    if hp >= 0:
        return 1 if hp <= 0xFF else 2 if hp <= 0xFFFF else 4
    return 1 if hp >= -128 else 2 if hp >= -32768 else 4


def staged_head_size(rec):
    """hostio.hpp staged_head_bytes(with_quals = true): the record as it lies in the BAM stream up to the end of its
    qualities -- block_size word | 32 bytes of fixed fields | name | CIGAR words | 4-bit bases | qualities"""
    l_seq = len(rec["seq"])
    return 4 + 32 + len(rec["name"]) + 1 + 4 * len(rec["cigar"]) + (l_seq + 1) // 2 + l_seq


def record_size(rec, n_final_ops):
    """bam_emit_kernels.hpp bam_record_size: a written record with its block_size word (no long CIGAR here)"""
    sl = rec["_sl"]
    return 36 + len(rec["name"]) + 1 + 4 * n_final_ops + (sl + 1) // 2 + sl + 3 + _hp_bytes(rec["hp"])


def words_class(n_words):
    return "0" if n_words == 0 else "1-63" if n_words < COPY_LANES else "64" if n_words == COPY_LANES else "65" if n_words == COPY_LANES + 1 else "66+"


def copy_call(what, dst, src, nib, clear_low, n):
    """wave_copy's split of one call: (what, dst & 3, src & 3, NIB, clear_low, min(n, head), n_words class, tail bytes)"""
    head = min(n, (4 - (dst & 3)) & 3)
    n_words = (n - head) >> 2
    return (what, dst & 3, src & 3, nib, clear_low, head, words_class(n_words), n - head - 4 * n_words)


def copy_calls(records, n_final_ops, batch_reads):
    """Every wave_copy call of emit_bam_records_kernel over the reads in batches of batch_reads, as copy_call() tuples, and
    the records' offsets in their batch.  Where source and destination lie is what the code does (align_engine.hpp,
    file_pipeline.hpp slot_pack_heads): a batch's staged heads lie back to back, without padding, from the start of an
    allocation (these reads are one group per batch: upload_group copies the slice to the buffer's start); the CIGAR words
    lie in slots at multiples of 4; the batch's records lie back to back from the start of the record buffer (the cursor is
    set to 0 with a batch's first group).  Allocations are aligned to more than 4."""
    calls, offsets = [], []
    for b0 in range(0, len(records), batch_reads):
        raw = out = 0
        for k in range(b0, min(len(records), b0 + batch_reads)):
            rec = records[k]
            lead, sl, l_seq = rec["_lead"], rec["_sl"], len(rec["seq"])
            l_rn, wl, nb = len(rec["name"]) + 1, 4 * n_final_ops[k], (sl + 1) // 2
            offsets.append(out)
            o = out + 36 + l_rn
            sq = raw + 36 + l_rn + 4 * len(rec["cigar"])
            calls.append(copy_call("cigar", o, 0, 0, False, wl))
            o += wl
            if sl > 0:
                calls.append(copy_call("bases", o, sq + (lead >> 1), lead & 1, bool(sl & 1), nb))
                o += nb
                if rec["qual"] is not None:
                    calls.append(copy_call("quals", o, sq + (l_seq + 1) // 2 + lead, 0, False, sl))
            raw += staged_head_size(rec)
            out += record_size(rec, n_final_ops[k])
    return calls, offsets
