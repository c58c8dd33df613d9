"""The coverage join of `analyze pileup_modbams --coverage-columns` restated in plain Python: per record mr.aligned_pairs and
the four rules, dictionaries of integers.  Shared by test_host_pileup_coverage.py (which asks it alone whether the synthetic
input is vacuous) and test_gpu_pileup_coverage.py (which compares the device's table with it).  Also the records that put
one edge case each on top of test_gpu_pileup._synthetic()."""
import modbam_restate as mr
import test_gpu_pileup as tp
import test_gpu_pileup_ref as tr

ALPHABET = tp.ALPHABET
REFS = tp.REFS
COLS = ("N_delete", "N_diff", "N_nocall")


def own_keys(rec, alphabet, region=None, genome=None, motifs=None, combine=False):
    """(status, the site keys of the record's kept calls - passing or fail): the emit's calls, through the motif test and the
    fold when there is a genome, then the region."""
    status, calls = tp.record_calls(rec, alphabet)
    if motifs is not None:
        calls = [c for c in (tr.place(c, genome, motifs, combine) for c in calls) if c is not None]
    return status, {c[:3] for c in calls if tp.in_region(c, region)}


def asked_position(site, reverse, genome, motifs, combine):
    """Where a record of that strand is asked about the site (ref_id, pos, strand), or None: not its strand, or - combined, a
    '-' record - no motif at the site."""
    rid, pos, strand = site
    if not combine:
        return pos if strand == int(reverse) else None
    if not reverse:
        return pos
    g = genome[rid]
    for motif, f in motifs:  # the first motif, in the order given, that matches the reference at the site
        s = pos - f
        if s >= 0 and s + len(motif) <= len(g) and all(tr.matches(g[s + i], motif[i]) for i in range(len(motif))):
            return pos + (len(motif) - 1 - 2 * f)
    return None


def record_cover(rec, alphabet, sites_of_contig, region=None, genome=None, motifs=None, combine=False):
    """{site: column} of one record over the sites of its contig: 0 delete, 1 diff, 2 nocall; a site it adds nothing to is
    not in the result."""
    status, own = own_keys(rec, alphabet, region, genome, motifs, combine)
    if status != 0:
        return {}
    reverse = bool(rec["flag"] & 0x10)
    canonical = "T" if alphabet[0] == "U" else alphabet[0]
    pairs = {r: (q, marker) for q, r, marker in mr.aligned_pairs(rec["cigar"], rec["pos"]) if r is not None}
    out = {}
    for site in sites_of_contig:
        rp = asked_position(site, reverse, genome, motifs, combine)
        if rp is None or rp not in pairs:  # outside the record's reference span
            continue
        if site in own:  # 1. a kept call: it is in the row already
            continue
        q, marker = pairs[rp]
        if q is None and marker is not None:  # 2. inside a D
            out[site] = 0
        elif q is not None:  # 3. an aligned base of the original read
            base = rec["seq"][q]
            base = mr.COMP.get(base, base) if reverse else base
            out[site] = 2 if ("T" if base == "U" else base) == canonical else 1
        # 4. an N skip: nothing
    return out


def cover_restate(records, alphabet, sites, region=None, genome=None, motifs=None, combine=False):
    """{site: [N_delete, N_diff, N_nocall]} for every site of `sites` (the keys of the restated table)."""
    by_contig = {}
    for site in sites:
        by_contig.setdefault(site[0], []).append(site)
    out = {site: [0, 0, 0] for site in sites}
    for rec in records:
        for site, col in record_cover(rec, alphabet, by_contig.get(rec["ref_id"], []), region, genome, motifs, combine).items():
            out[site][col] += 1
    return out


def bed18_text(table, cover, alphabet, refs, min_coverage=1, combine=False):
    out = []
    for (rid, pos, strand), row in sorted(table.items()):
        nv = sum(row[:-1])
        if nv < max(min_coverage, 1):
            continue
        cov = cover[(rid, pos, strand)]
        for j, code in enumerate(alphabet[1:]):
            cols = [refs[rid][0], pos, pos + 1, code, min(nv, 1000), "." if combine else "+-"[strand], pos, pos + 1, "255,0,0", nv,
                    f"{100 * row[1 + j] / nv:.2f}", row[1 + j], row[0], nv - row[1 + j] - row[0], cov[0], row[-1], cov[1], cov[2]]
            out.append("\t".join(map(str, cols)) + "\n")
    return "".join(out)


def tsv_text(table, cover, alphabet, refs, combine=False):
    head = "\t".join(["chrom", "start", "strand"] + [f"N_{a}" for a in alphabet] + ["N_fail"] + list(COLS)) + "\n"
    return head + "".join(f"{refs[rid][0]}\t{pos}\t{'.' if combine else '+-'[strand]}\t" + "\t".join(map(str, row + cover[(rid, pos, strand)])) + "\n"
                          for (rid, pos, strand), row in sorted(table.items()))


# ---- the input: test_gpu_pileup._synthetic() and one small record per edge case -------------------------------------------------
def _called(seq, cigar, positions, ml, flag=0, ref=0, pos=0, code="m", name=None, base="C"):
    """A record whose MM tag lists the `base` at `positions` of the ORIGINAL sequence (ascending) with `code`."""
    orig = mr.original_sequence(seq, bool(flag & 16))
    cs = [i for i, b in enumerate(orig) if b == base]
    ordinals = [cs.index(p) for p in positions]
    deltas = [o - (ordinals[k - 1] + 1 if k else 0) for k, o in enumerate(ordinals)]
    rec = tp._rec(seq, cigar, f"{base}+{code}?" + "".join(f",{d}" for d in deltas) + ";", list(ml), flag=flag, ref=ref, pos=pos)
    rec["case"] = name
    return rec


def over(pos, seq, cigar, site_pos, flag=0, ref=0, base="C", code="m"):
    """A status-0 record with ONE kept call, of `code`, on an aligned `base` away from reference position `site_pos`."""
    reverse = bool(flag & 16)
    orig = mr.original_sequence(seq, reverse)
    q2r = {q: r for q, r, _ in mr.aligned_pairs(cigar, pos) if q is not None and r is not None}
    stored = lambda i: len(seq) - 1 - i if reverse else i  # noqa: E731
    call = next(i for i, b in enumerate(orig) if b == base and q2r.get(stored(i), site_pos) != site_pos)
    return _called(seq, cigar, [call], [250], flag=flag, ref=ref, pos=pos, code=code, base=base)


def edge_records(genome):
    """One small record per case of the issue, named in `case`; and {case: (site, what the record adds there)} - the column, or
    None for nothing - which the host test asks of the restatement.  The sites are positions that reads of _synthetic() call."""
    g = genome[0]
    recs, expect = [], {}

    def add(rec, case, site, col):
        rec["case"] = case
        recs.append(rec)
        expect[case] = (site, col)

    def base_at(lo, hi, base="C"):  # a reference position in [lo, hi) of contig 0 holding that base
        return next(p for p in range(lo, hi) if g[p] == base)

    # the first and the last reference position of a record; one base before and one behind its span
    first, last = base_at(1000, 1100), base_at(1100, 1200)
    add(over(first, g[first : first + 60], [("M", 60)], first), "first_position", (0, first, 0), 2)
    add(over(last - 59, g[last - 59 : last + 1], [("M", 60)], last), "last_position", (0, last, 0), 2)
    add(over(first + 1, g[first + 1 : first + 61], [("M", 60)], first), "one_before_the_span", (0, first, 0), None)
    add(over(last - 60, g[last - 60 : last], [("M", 60)], last), "one_behind_the_span", (0, last, 0), None)
    # inside a D; the last M base before it and the first behind it
    d = base_at(1250, 1300)
    add(over(d - 30, g[d - 30 : d - 1] + g[d + 2 : d + 32], [("M", 29), ("D", 3), ("M", 30)], d), "inside_a_deletion", (0, d, 0), 0)
    add(over(d - 20, g[d - 20 : d + 1] + g[d + 3 : d + 33], [("M", 21), ("D", 2), ("M", 30)], d), "last_base_before_a_deletion", (0, d, 0), 2)
    add(over(d - 22, g[d - 22 : d - 2] + g[d : d + 30], [("M", 20), ("D", 2), ("M", 30)], d), "first_base_behind_a_deletion", (0, d, 0), 2)
    # beside an insertion and beside a soft clip
    add(over(d - 20, g[d - 20 : d + 1] + "TTT" + g[d + 1 : d + 31], [("M", 21), ("I", 3), ("M", 30)], d), "beside_an_insertion", (0, d, 0), 2)
    add(over(d, "TTTT" + g[d : d + 40], [("S", 4), ("M", 40)], d), "beside_a_soft_clip", (0, d, 0), 2)
    # inside an N skip
    add(over(d - 30, g[d - 30 : d - 1] + g[d + 2 : d + 32], [("M", 29), ("N", 3), ("M", 30)], d), "inside_a_skip", (0, d, 0), None)
    # flag 0x10: the stored base is the complement of the canonical base (nocall), or something else (diff)
    gpos = base_at(1400, 1500, "G")  # a '-'-strand site of the synthetic reads
    add(over(gpos - 20, g[gpos - 20 : gpos + 30], [("M", 50)], gpos, flag=16), "reverse_stored_complement", (0, gpos, 1), 2)
    add(over(gpos - 20, g[gpos - 20 : gpos] + "T" + g[gpos + 1 : gpos + 30], [("M", 50)], gpos, flag=16), "reverse_stored_other", (0, gpos, 1), 1)
    # a read base N
    n_at = base_at(1500, 1600)
    add(over(n_at - 20, g[n_at - 20 : n_at] + "N" + g[n_at + 1 : n_at + 30], [("M", 50)], n_at), "read_base_n", (0, n_at, 0), 1)
    # a failing call at the site: nothing beyond N_fail (ML 128 of m: kmax = 257 of 512, fails at a threshold of 0.8)
    f_at = base_at(1600, 1700)
    add(_called(g[f_at : f_at + 40], [("M", 40)], [0], [128], pos=f_at), "failing_call", (0, f_at, 0), None)
    # the only entry at the site has a code outside the alphabet (nocall); the record counts through its entry of m on the next C
    add(tp._rec(g[f_at : f_at + 40], [("M", 40)], "C+a?,0;C+m?,1;", [200, 250], pos=f_at), "code_outside_the_alphabet", (0, f_at, 0), 2)
    # status 0, none of its calls kept: its only call lies under a soft clip
    add(_called("C" + g[f_at : f_at + 40], [("S", 1), ("M", 40)], [0], [250], pos=f_at), "no_call_kept", (0, f_at, 0), 2)
    # every non-zero status over a site
    seq, site = g[f_at - 10 : f_at + 30], (0, f_at, 0)
    add(tp._rec(seq, [("M", 40)], None, None, pos=f_at - 10), "status_1", site, None)
    add(tp._rec(seq, [("M", 40)], "C+m?,x;", [1], pos=f_at - 10), "status_2", site, None)
    add(tp._rec(seq, [("M", 40)], "C+m?,0;", [200], flag=4, pos=f_at - 10), "status_3", site, None)
    add(tp._rec(seq, [("M", 40)], "C+a?,0;", [200], pos=f_at - 10), "status_5", site, None)
    add(tp._rec(seq, [("M", 40)], "C+m?,0;", [200], flag=0x100, pos=f_at - 10), "status_6", site, None)
    # two contigs with a site at one position: a call on each, and a record over each
    both = next(p for p in range(1700, 1800) if g[p] == "C" and genome[1][p] == "C")
    for ref in (0, 1):
        add(_called(genome[ref][both : both + 30], [("M", 30)], [0], [250], ref=ref, pos=both), f"same_position_contig_{ref}", (ref, both, 0), None)
        add(over(both - 25, genome[ref][both - 25 : both + 25], [("M", 50)], both, ref=ref), f"over_same_position_contig_{ref}", (ref, both, 0), 2)
    # both strands at that position: a '-' record whose original sequence has a C there (its stored base a G)
    add(_called(g[both - 29 : both] + "G", [("M", 30)], [0], [250], flag=16, pos=both - 29), "both_strands_at_one_position", (0, both, 1), None)
    add(over(both - 25, g[both - 25 : both + 25], [("M", 50)], both, flag=16), "minus_over_both_strands", (0, both, 1), 1)
    # a deletion over a site and a substituted base on a site, on every contig and strand
    swap = {"A": "C", "C": "A", "G": "T", "T": "G"}
    for ref in (0, 1):
        for rev in (False, True):
            gr, base = genome[ref], "G" if rev else "C"
            p = next(p for p in range(400, 500) if gr[p] == base)
            s = next(s for s in range(p + 10, 600) if gr[s] == base)
            seq = gr[p - 40 : p] + gr[p + 3 : s] + swap[base] + gr[s + 1 : s + 40]
            rec = over(p - 40, seq, [("M", 40), ("D", 3), ("M", s + 40 - p - 3)], p, flag=16 if rev else 0, ref=ref)
            add(rec, f"deletion_contig_{ref}_{'-' if rev else '+'}", (ref, p, int(rev)), 0)
            add(dict(rec), f"substitution_contig_{ref}_{'-' if rev else '+'}", (ref, s, int(rev)), 1)
            # and at the deleted site a substituted base and an uncalled canonical one: a site with all three columns
            rec = over(p - 30, gr[p - 30 : p] + swap[base] + gr[p + 1 : p + 30], [("M", 60)], p, flag=16 if rev else 0, ref=ref)
            add(rec, f"substitution_at_the_deleted_site_{ref}_{'-' if rev else '+'}", (ref, p, int(rev)), 1)
            rec = over(p - 30, gr[p - 30 : p + 30], [("M", 60)], p, flag=16 if rev else 0, ref=ref)
            add(rec, f"uncalled_at_the_deleted_site_{ref}_{'-' if rev else '+'}", (ref, p, int(rev)), 2)
    return recs, expect


def coverage_input():
    """(records, genome, {case: (site, column or None)}): _synthetic() and the edge records."""
    recs, genome = tp._synthetic()
    edges, expect = edge_records(genome)
    return recs + edges, genome, expect
