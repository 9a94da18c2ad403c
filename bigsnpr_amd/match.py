"""snp_match and same_ref — host mirrors of R/match-alleles.R.  Tables are mappings from column name to equal-length
arrays (the reference's data frames); row numbers are 0-based."""
import numpy as np

_FLIP = {"A": "T", "C": "G", "T": "A", "G": "C"}
_AMBIGUOUS = {("A", "T"), ("T", "A"), ("C", "G"), ("G", "C")}


def flip_strand(allele):
    """R/match-alleles.R:3-14: A <-> T, C <-> G, anything else has no twin (None)"""
    return [_FLIP.get(a) for a in allele]


def _table(t, what):
    try:
        cols = {str(k): np.asarray(v) for k, v in dict(t).items()}
    except (TypeError, ValueError):
        raise TypeError("'%s' should map column names to columns." % what)
    sizes = {v.shape[0] if v.ndim else 1 for v in cols.values()}
    if len(sizes) > 1:
        n = max(sizes)
        if sizes != {1, n}:
            raise ValueError("Incompatibility between dimensions.")
        cols = {k: (np.repeat(v.ravel(), n) if v.size == 1 else v) for k, v in cols.items()}   # data.frame(chr = 1, ...)
    return cols, (max(sizes) if sizes else 0)


def _key(v):
    """a hashable join value; a missing one (None, NaN) matches nothing"""
    if v is None:
        return None
    if isinstance(v, (float, np.floating)):
        if v != v:
            return None
        return int(v) if float(v).is_integer() else float(v)
    if isinstance(v, (int, np.integer)):
        return int(v)
    return str(v)


def _fmt(n):
    return format(int(n), ",")      # format(., big.mark = ",")


def snp_match(sumstats, info_snp, strand_flip=True, join_by_pos=True, remove_dups=True, match_min_prop=0.2,
              return_flip_and_rev=False, verbose=True):
    """R/match-alleles.R:50-130.  Match by ("chr", "a0", "a1") and ("pos" or "rsid"), accounting for strand flips and
    reversed reference alleles; `beta` is negated where the alleles are reversed.  Returns a mapping with the matched
    rows ordered by (chr, pos): the join columns, the other columns of `sumstats` (suffix ".ss" where `info_snp` has
    the name too), the other columns of `info_snp`; "_NUM_ID_.ss" and "_NUM_ID_" are the 0-based rows of the inputs."""
    def message2(fmt, *a):
        if verbose:
            print(fmt % a)

    ss, n_ss = _table(sumstats, "sumstats")
    info, n_info = _table(info_snp, "info_snp")
    ss["_NUM_ID_"] = np.arange(n_ss)
    info["_NUM_ID_"] = np.arange(n_info)
    min_match = match_min_prop * min(n_ss, n_info)

    join_by = ["chr", "pos" if join_by_pos else "rsid", "a0", "a1"]
    if not all(c in ss for c in join_by + ["beta"]):
        raise ValueError("Please use proper names for variables in 'sumstats'. Expected '%s'."
                         % ", ".join(join_by + ["beta"]))
    if not all(c in info for c in join_by + ["pos"]):
        raise ValueError("Please use proper names for variables in 'info_snp'. Expected '%s'."
                         % ", ".join(list(dict.fromkeys(join_by + ["pos"]))))

    message2("%s variants to be matched.", _fmt(n_ss))

    # first filter (to fasten)
    k1, k2 = join_by[0], join_by[1]
    there = {(_key(c), _key(p)) for c, p in zip(info[k1].tolist(), info[k2].tolist())}
    rows = [i for i, (c, p) in enumerate(zip(ss[k1].tolist(), ss[k2].tolist()))
            if _key(c) is not None and _key(p) is not None and (_key(c), _key(p)) in there]
    if not rows:
        raise ValueError("No variant has been matched.")

    a0 = [None if a is None else str(a) for a in ss["a0"].tolist()]
    a1 = [None if a is None else str(a) for a in ss["a1"].tolist()]
    # candidates (row of sumstats, a0, a1, flipped): as given, and on the other strand
    cand = []
    if strand_flip:
        ambiguous = [i for i in rows if (a0[i], a1[i]) in _AMBIGUOUS]
        message2("%s ambiguous SNPs have been removed.", _fmt(len(ambiguous)))
        drop = set(ambiguous)
        rows = [i for i in rows if i not in drop]
        cand += [(i, a0[i], a1[i], False) for i in rows]
        cand += [(i, _FLIP.get(a0[i]), _FLIP.get(a1[i]), True) for i in rows]
    else:
        cand += [(i, a0[i], a1[i], False) for i in rows]
    # ... and each with the alleles swapped (the effect changes sign)
    cand = [c + (False,) for c in cand] + [(i, y, x, f, True) for i, x, y, f in cand]

    index = {}
    for j, key in enumerate(zip(info[k1].tolist(), info[k2].tolist(), info["a0"].tolist(), info["a1"].tolist())):
        key = tuple(_key(v) for v in key)
        if None not in key:
            index.setdefault(key, []).append(j)
    pairs = []                                  # (join key, candidate order, row of sumstats, row of info_snp, flip, rev)
    for o, (i, x, y, f, r) in enumerate(cand):
        key = (_key(ss[k1][i]), _key(ss[k2][i]), x, y)
        if None in key:
            continue
        for j in index.get(key, ()):
            pairs.append((key, o, i, j, f, r))
    # merge() returns its rows sorted by the join columns; (chr, pos) is sorted last, below, and is stable over this
    pairs.sort(key=lambda t: ("" if join_by_pos else str(t[0][1]), t[0][2], t[0][3], t[1], t[3]))

    if remove_dups and pairs:
        seen = {}
        for t in pairs:
            pos = (_key(info["chr"][t[3]]), _key(info["pos"][t[3]]))
            seen[pos] = seen.get(pos, 0) + 1
        kept = [t for t in pairs if seen[(_key(info["chr"][t[3]]), _key(info["pos"][t[3]]))] == 1]
        if len(kept) < len(pairs):
            pairs = kept
            message2("Some duplicates were removed.")

    message2("%s variants have been matched; %s were flipped and %s were reversed.", _fmt(len(pairs)),
             _fmt(sum(t[4] for t in pairs)), _fmt(sum(t[5] for t in pairs)))
    if len(pairs) < min_match:
        raise ValueError("Not enough variants have been matched.")

    i_ss = np.array([t[2] for t in pairs], dtype=np.int64)
    i_info = np.array([t[3] for t in pairs], dtype=np.int64)
    flip = np.array([t[4] for t in pairs], dtype=bool)
    rev = np.array([t[5] for t in pairs], dtype=bool)
    # order(chr, pos), stable over the join order
    chr_, pos_ = info["chr"][i_info], info["pos"][i_info]
    order = np.lexsort((np.arange(i_ss.size), pos_, chr_)) if i_ss.size else np.arange(0)
    i_ss, i_info, flip, rev = i_ss[order], i_info[order], flip[order], rev[order]

    out = {}
    for c in join_by:                           # the join columns carry info_snp's (equal) values
        out[c] = info[c][i_info]
    for c, v in ss.items():
        if c in join_by:
            continue
        col = v[i_ss]
        if c == "beta":
            col = np.where(rev, -col.astype(np.float64), col.astype(np.float64))
        out[c + ".ss" if c in info else c] = col
    if return_flip_and_rev:
        out["_FLIP_"], out["_REV_"] = flip, rev
    for c, v in info.items():
        if c not in join_by:
            out[c] = v[i_info]
    return out


def same_ref(ref1, alt1, ref2, alt2):
    """R/match-alleles.R:156-200: whether the reference alleles of two datasets are the same, accounting for strand
    flips (this does NOT remove ambiguous alleles).  An object array of True / False / None: None where an allele is
    missing or not one of A, C, G, T, where a dataset has ref == alt, and where the pairs cannot be matched."""
    def one(r1, a1, r2, a2):
        if any(x not in _FLIP for x in (r1, a1, r2, a2)) or r1 == a1 or r2 == a2:
            return None
        if r1 == r2 and a1 == a2:
            return True
        if r1 == a2 and a1 == r2:
            return False
        if _FLIP[r1] == r2 and _FLIP[a1] == a2:
            return True
        if _FLIP[r1] == a2 and _FLIP[a1] == r2:
            return False
        return None

    cols = [np.asarray(x, dtype=object).ravel().tolist() for x in (ref1, alt1, ref2, alt2)]
    if len({len(c) for c in cols}) != 1:
        raise ValueError("Incompatibility between dimensions.")
    res = np.empty(len(cols[0]), dtype=object)
    res[:] = [one(*t) for t in zip(*cols)]
    return res
