"""NM and the short-form cs difference string of one alignment record, restated in plain Python from the grammar of minimap2's
manual page (--cs): `:<n>` identical columns, `*<ref><query>` a substitution, `+<bases>` an insertion, `-<bases>` a deletion, bases
lower case, clips not represented, a run of identical columns ends with its M op.  An N (anything but ACGT / acgt) on either side
pairs with nothing: the column is a substitution written with `n` and counts in NM."""

M, I, D, S, H = 0, 1, 2, 4, 5
_COMP = str.maketrans("ACGTNacgtn", "TGCANtgcan")


def revcomp(s: str) -> str:
    return s.translate(_COMP)[::-1]


def _base(c: str) -> str:
    c = c.lower()
    return c if c in "acgt" else "n"


def cs_nm(cigar, query: str, ref: str, ref_start: int = 0):
    """cigar: [(op, len)] over the whole strand-oriented query (clips included); ref: the window -> (nm, cs)"""
    q, t, nm, out = 0, ref_start, 0, []
    for op, n in cigar:
        if op == M:
            run = 0
            for a, b in zip(query[q:q + n], ref[t:t + n]):
                a, b = _base(a), _base(b)
                if a == b and a != "n":
                    run += 1
                    continue
                if run:
                    out.append(":%d" % run)
                out.append("*" + b + a)
                run, nm = 0, nm + 1
            if run:
                out.append(":%d" % run)
            q, t = q + n, t + n
        elif op == I and n:
            out.append("+" + "".join(_base(c) for c in query[q:q + n]))
            q, nm = q + n, nm + n
        elif op == D and n:
            out.append("-" + "".join(_base(c) for c in ref[t:t + n]))
            t, nm = t + n, nm + n
        elif op in (S, H):
            q += n
    return nm, "".join(out)
