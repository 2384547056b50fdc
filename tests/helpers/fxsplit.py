"""TEST INFRASTRUCTURE: the host model of smr_fastx_split.  expected_streams(reads, hits, opts) -> eight bytes objects, aligned[0..3] then
other[0..3]: what the report writer puts into aligned.* / other.* when it is given the reads in order.  The three strings of a record are the
host parser's (Reads.record_text of Reads.from_fastx_text), the record is write_fx's (header, letters, for FASTQ "+" and quality, each followed
by a newline), the routing restates smr_report_add and the table of smr_report_add_pair (csrc/smr_report.cpp).  test_fxsplit_model.py pins
this model to the writer itself."""

VALID_OPTS = [dict(paired_in=pi, paired_out=po, out2=o2, sout=so)
              for pi, po, o2, so in [(0, 0, 0, 0), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (1, 0, 1, 0), (0, 1, 1, 0), (0, 0, 0, 1), (0, 0, 1, 1)]]


def opts_id(o):
    return "+".join(k for k in ("paired_in", "paired_out", "out2", "sout") if o.get(k)) or "plain"


def record_bytes(reads, i):
    hdr, seq, qual = reads.record_text(i)
    out = hdr.encode() + b"\n" + seq.encode() + b"\n"
    if reads.is_fastq:
        out += b"+\n" + qual.encode() + b"\n"
    return out


def num_out(o):
    return 4 if (o.get("out2") and o.get("sout")) else 2 if (o.get("out2") or o.get("sout")) else 1


def pair_files(o, hit):
    """-> ([aligned file of mate 0, of mate 1], [other file of mate 0, of mate 1]), None = not written"""
    both, any_ = hit[0] and hit[1], hit[0] or hit[1]
    n = num_out(o)
    al, ot = [None, None], [None, None]
    if any_:
        for i in range(2):
            if n == 1:
                if (both if o.get("paired_out") else (o.get("paired_in") or hit[i])):
                    al[i] = 0
            elif n == 2 and o.get("out2"):
                if o.get("paired_out"):
                    if not both:
                        break
                    al[i] = i
                elif o.get("paired_in") or hit[i]:
                    al[i] = i
            elif n == 2:
                al[i] = 0 if both else 1 if hit[i] else None
            else:
                al[i] = i if both else i + 2 if hit[i] else None
    if not both:
        for i in range(2):
            if n == 1:
                if ((not any_) if o.get("paired_in") else (o.get("paired_out") or not hit[i])):
                    ot[i] = 0
            elif n == 2 and o.get("out2"):
                if o.get("paired_in"):
                    if any_:
                        break
                    ot[i] = i
                elif o.get("paired_out") or not hit[i]:
                    ot[i] = i
            elif n == 2:
                ot[i] = 0 if not any_ else 1 if not hit[i] else None
            else:
                ot[i] = i if not any_ else i + 2 if not hit[i] else None
    return al, ot


def expected_streams(reads, hits, opts):
    """reads: a Reads with its text (layouts 0 and 1), or (reads, mates) for layout 2; hits: one truth value per read, those of `reads`, then
    those of `mates`; opts: dict(layout, paired_in, paired_out, out2, sout, aligned, other) -- what Engine.fastx_split takes"""
    layout = opts.get("layout", 0)
    want = [opts.get("aligned", True)] * 4 + [opts.get("other", True)] * 4
    out = [[] for _ in range(8)]
    if layout == 0:
        for i in range(reads.count):
            out[0 if hits[i] else 4].append(record_bytes(reads, i))
    else:
        a, b = reads if layout == 2 else (reads, reads)
        n_pairs = a.count if layout == 2 else a.count // 2
        for k in range(n_pairs):
            idx = [k, k] if layout == 2 else [2 * k, 2 * k + 1]
            hit = [bool(hits[k]), bool(hits[a.count + k])] if layout == 2 else [bool(hits[2 * k]), bool(hits[2 * k + 1])]
            al, ot = pair_files(opts, hit)
            for i, src in enumerate((a, b)):
                if al[i] is not None:
                    out[al[i]].append(record_bytes(src, idx[i]))
                if ot[i] is not None:
                    out[4 + ot[i]].append(record_bytes(src, idx[i]))
    return [b"".join(x) if want[k] else b"" for k, x in enumerate(out)]
