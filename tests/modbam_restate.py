"""Plain-Python restatement of the rules of `validate from_modbams` (MM / ML grammar, the walk along the original sequence,
the CIGAR walk, the truth lookup), written from the specification and not from the kernel, plus helpers that build BAM
records by hand.  The GPU tests compare remora_amd against it; tools/gen_golden.py builds its duck-typed pysam reads from it;
tests/manual/prof_modbams.py times it."""
import re
import struct

import numpy as np

ENTRY = re.compile(r"([ACGTUN])([+-])([a-z]+|[0-9]+)([.?]?)((?:,[0-9]+)*);")
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
OK, NO_MM, MALFORMED, UNMAPPED, NO_MD, NO_VALID = 0, 1, 2, 3, 4, 5


class Malformed(Exception):
    pass


def parse_mm_ml(mm, ml):
    """[(base, strand, codes, flag, deltas, ml rows [n_deltas][n_codes])] of an MM string and its ML values (None: absent)."""
    entries, at, used = [], 0, 0
    while at < len(mm):
        m = ENTRY.match(mm, at)
        if m is None:
            raise Malformed(mm[at:])
        base, strand, code, flag, dl = m.groups()
        codes = list(code) if code[0].isalpha() else [int(code)]
        deltas = [int(d) for d in dl.split(",")[1:]]
        need = len(codes) * len(deltas)
        if need and (ml is None or used + need > len(ml)):
            raise Malformed("ML too short")
        rows = [[int(ml[used + k * len(codes) + c]) for c in range(len(codes))] for k in range(len(deltas))]
        used += need
        entries.append((base, strand, codes, flag, deltas, rows))
        at = m.end()
    if ml is not None and used != len(ml):
        raise Malformed("ML too long")
    return entries


def original_sequence(seq, reverse):
    return "".join(COMP.get(b, b) for b in reversed(seq)) if reverse else seq


def entry_positions(seq, reverse, base, deltas):
    """Stored-coordinate position of every call of one entry; Malformed when a call lies beyond the last occurrence."""
    orig = original_sequence(seq, reverse)
    want = "T" if base == "U" else base
    occ = [p for p, b in enumerate(orig) if want == "N" or b == want]
    out, ordinal = [], -1
    for d in deltas:
        ordinal += d + 1
        if ordinal >= len(occ):
            raise Malformed("call beyond the last occurrence")
        out.append(len(seq) - 1 - occ[ordinal] if reverse else occ[ordinal])
    return out


def modified_bases(seq, reverse, mm, ml):
    """pysam's AlignedSegment.modified_bases restated: {(base, strand, code): [(stored position, ML value)]}; the strand of the
    key is flipped for a reverse record.  None without an MM tag."""
    if mm is None:
        return None
    out = {}
    for base, strand, codes, _, deltas, rows in parse_mm_ml(mm, ml):
        pos = entry_positions(seq, reverse, base, deltas)
        for c, code in enumerate(codes):
            key = (base, int((strand == "-") != bool(reverse)), code)
            out.setdefault(key, [])
            out[key] = out[key] + [(p, row[c]) for p, row in zip(pos, rows)]
    return out


def aligned_pairs(cigar, pos, has_md=True):
    """get_aligned_pairs(with_seq=True) restated from the CIGAR: (query position, reference position, reference base) per
    column; the base is only a marker here (nothing reads its value).  ValueError without an MD tag, as pysam."""
    if not has_md:
        raise ValueError("MD tag not present")
    q, r, out = 0, pos, []
    for op, n in cigar:
        if op in "M=X":
            out += [(q + i, r + i, "N") for i in range(n)]
            q, r = q + n, r + n
        elif op in "IS":
            out += [(q + i, None, None) for i in range(n)]
            q += n
        elif op == "D":
            out += [(None, r + i, "N") for i in range(n)]
            r += n
        elif op == "N":
            out += [(None, r + i, None) for i in range(n)]
            r += n
    return out


def join_record(rec, alphabet, gt_sites):
    """One record (dict: seq, flag, ref_id, ref_name, pos, cigar [(op, n)], mm, ml, has_md) ->
    (status, probs [n][len(alphabet)], labels, qpos, rpos) by the rules of the specification."""
    none = ([], [], [], [])
    reverse = bool(rec["flag"] & 0x10)
    seq = rec["seq"]
    if rec["mm"] is None:
        return (NO_MM,) + none
    try:
        entries = parse_mm_ml(rec["mm"], rec["ml"])
    except Malformed:
        return (MALFORMED,) + none
    if rec["ref_id"] < 0:
        return (UNMAPPED,) + none
    if not rec["has_md"]:
        return (NO_MD,) + none
    mods = list(alphabet[1:])
    if not any(strand == "+" and any(c in mods for c in codes) for _, strand, codes, _, _, _ in entries):
        return (NO_VALID,) + none
    if sum(n for op, n in rec["cigar"] if op in "MIS=X") != len(seq):
        return (MALFORMED,) + none
    called = {}
    try:
        for base, strand, codes, _, deltas, rows in entries:
            pos = entry_positions(seq, reverse, base, deltas)  # every entry is walked: any call beyond the end is malformed
            if strand != "+":
                continue
            for p, row in zip(pos, rows):
                for code, q in zip(codes, row):
                    if code in mods:
                        called.setdefault(p, {})[code] = (q + 0.5) / 256  # the later entry wins
    except Malformed:
        return (MALFORMED,) + none
    q2r = {q: r for q, r, _ in aligned_pairs(rec["cigar"], rec["pos"]) if q is not None and r is not None}
    truth = gt_sites.get((rec["ref_name"], "-" if reverse else "+"), {})
    probs, labels, qpos, rpos = [], [], [], []
    for p in sorted(called):
        r = q2r.get(p)
        if r is None or r not in truth:
            continue
        row = [called[p].get(m, 0.0) for m in mods]
        probs.append([1 - sum(row)] + row)
        labels.append(alphabet.index(truth[r]))
        qpos.append(p)
        rpos.append(r)
    return OK, probs, labels, qpos, rpos


def join_records(records, alphabet, gt_sites):
    """join_record over a file: (probs f64[n][a], labels i64[n], qpos, rpos, counts per record, status per record)."""
    parts = [join_record(rec, alphabet, gt_sites) for rec in records]
    cat = lambda i, dt, w: (np.concatenate([np.asarray(p[i], dt).reshape(-1, *w) for p in parts]) if parts  # noqa: E731
                            else np.zeros((0, *w), dt))
    return (cat(1, np.float64, (len(alphabet),)), cat(2, np.int64, ()), cat(3, np.int64, ()), cat(4, np.int64, ()),
            np.array([len(p[2]) for p in parts], np.int64), np.array([p[0] for p in parts], np.int32))


# ---- BAM records by hand -------------------------------------------------------------------------------------------------
_NT16 = {c: i for i, c in enumerate("=ACMGRSVTWYHKDBN")}
_CIG = {c: i for i, c in enumerate("MIDNSHP=X")}


def mod_tags(mm, ml, lower=False):
    """Tag bytes of an MM:Z / ML:B:C pair (None: that tag is left out); `lower`: the Mm / Ml spellings."""
    out = b""
    if mm is not None:
        out += (b"MmZ" if lower else b"MMZ") + mm.encode() + b"\x00"
    if ml is not None:
        out += (b"MlBC" if lower else b"MLBC") + struct.pack("<i", len(ml)) + bytes(ml)
    return out


def bam_record(name, flag, ref_id, pos, cigar, seq, tags=b"", has_md=True, mapq=60):
    """A stored record with its block_size in front.  cigar: [(op letter, length)]."""
    nib = [_NT16[c] for c in seq] + ([0] if len(seq) % 2 else [])
    packed = bytes((nib[i] << 4) | nib[i + 1] for i in range(0, len(nib), 2))
    nm = name.encode() + b"\x00"
    body = struct.pack("<iiBBHHHiiii", ref_id, pos, len(nm), mapq, 4680, len(cigar), flag, len(seq), -1, -1, 0) + nm
    body += b"".join(struct.pack("<I", (n << 4) | _CIG[op]) for op, n in cigar) + packed + b"\xff" * len(seq)
    body += (b"MDZ" + str(len(seq)).encode() + b"\x00" if has_md else b"") + tags
    return struct.pack("<i", len(body)) + body


def bam_header(refs):
    """Header bytes for [(name, length)]."""
    text = "@HD\tVN:1.6\tSO:unsorted\n" + "".join(f"@SQ\tSN:{n}\tLN:{ln}\n" for n, ln in refs)
    out = b"BAM\x01" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(refs))
    for n, ln in refs:
        out += struct.pack("<i", len(n) + 1) + n.encode() + b"\x00" + struct.pack("<i", ln)
    return out


def write_bam(path, refs, records):
    """records: dicts as join_record takes them (plus `name`, optional `tags_lower`) -> a BAM file through BamWriter."""
    from remora_amd.io import BamWriter

    with BamWriter(str(path), bam_header(refs), threads=1) as w:
        for i, rec in enumerate(records):
            w.write(bam_record(rec.get("name", f"read{i}"), rec["flag"], rec["ref_id"], rec["pos"], rec["cigar"], rec["seq"],
                               mod_tags(rec["mm"], rec["ml"], rec.get("tags_lower", False)), rec["has_md"]))
