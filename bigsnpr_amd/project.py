"""bed_projectPCA — host mirror of R/bed-projectPCA.R:100-172: match the variants of a reference and a target .bed file,
compute the (auto) SVD of the reference, and project the target on it (simple and OADP projections) in one library
call (bsn_bed_project_pca): no linear algebra runs on the host after the SVD."""
import numpy as np

from .autosvd import bed_autoSVD
from .bed import _check_ind, assert_bed
from .match import snp_match
from .prs import project_pca


def _bim_map(obj_bed):
    """setNames(obj.bed$map[-3], c("chr", "rsid", "pos", "a1", "a0"))"""
    m = obj_bed.map
    return dict(chr=m["chromosome"], rsid=m["marker_ID"], pos=m["physical_pos"], a1=m["allele1"], a0=m["allele2"])


def bed_projectPCA(obj_bed_ref, obj_bed_new, k=10, ind_row_new=None, ind_row_ref=None, ind_col_ref=None,
                   strand_flip=True, join_by_pos=True, match_min_prop=0.5, build_new="hg19", build_ref="hg19",
                   liftOver=None, verbose=True, **autosvd_args):
    """R/bed-projectPCA.R:100-172.  Returns dict(obj_svd_ref, simple_proj, OADP_proj).  `autosvd_args` go to bed_autoSVD
    (fun_scaling, thr_r2, size, roll_size, int_min_size, alpha_tukey, min_mac, min_maf, max_iter, ncores).

    A variant whose alleles are reversed in the target enters with centre' = (centre - 1) beta + 1 and
    scale' = scale beta, beta = -1: (g - centre') / scale' = ((2 - g) - centre) / scale.  A strand flip changes the
    letters, not the genotypes."""
    def printf2(fmt, *a):
        if verbose:
            print(fmt % a, end="")

    assert_bed(obj_bed_ref)
    assert_bed(obj_bed_new)
    for name in ("obj_bed", "ind_row", "ind_col", "k", "verbose"):
        if name in autosvd_args:
            raise TypeError("bed_projectPCA() sets '%s' of bed_autoSVD() itself." % name)

    printf2("\n[Step 1/3] Matching variants of reference with target data..\n")
    map_ref, map_new = _bim_map(obj_bed_ref), _bim_map(obj_bed_new)
    if join_by_pos and build_new != build_ref:
        if liftOver is None:
            raise ValueError("Please provide path to liftOver executable.")
        raise NotImplementedError("liftOver is an external executable, not emulated: convert the positions of the "
                                  "target to build '%s' beforehand." % build_ref)
    info_snp = snp_match(dict(map_ref, beta=1.0), map_new, strand_flip=strand_flip, join_by_pos=join_by_pos,
                         match_min_prop=match_min_prop, verbose=verbose)

    printf2("\n[Step 2/3] Computing (auto) SVD of reference..\n")
    ref_id = np.asarray(info_snp["_NUM_ID_.ss"], dtype=np.int64)
    matched = np.zeros(obj_bed_ref.ncol, dtype=bool)
    matched[ref_id] = True
    if ind_col_ref is None:
        ind_col = np.nonzero(matched)[0]
    else:                                                  # intersect(): the order of ind.col.ref, without repeats
        icr = _check_ind("ind.col.ref", ind_col_ref, obj_bed_ref.ncol)
        _, first = np.unique(icr, return_index=True)
        icr = icr[np.sort(first)]
        ind_col = icr[matched[icr]]
    obj_svd = bed_autoSVD(obj_bed_ref, ind_row=ind_row_ref, ind_col=ind_col, k=k, verbose=verbose, **autosvd_args)

    printf2("\n[Step 3/3] Projecting PC scores on new data..\n")
    where = np.full(obj_bed_ref.ncol, -1, dtype=np.int64)
    where[ref_id[::-1]] = np.arange(ref_id.size)[::-1]      # match(): the first occurrence
    keep = where[np.asarray(obj_svd["subset"], dtype=np.int64)]
    beta = np.asarray(info_snp["beta"], dtype=np.float64)[keep]
    ind_row_new = np.arange(obj_bed_new.nrow) if ind_row_new is None else ind_row_new
    XV, _, oadp = project_pca(obj_bed_new, ind_row_new, np.asarray(info_snp["_NUM_ID_"], dtype=np.int64)[keep],
                              (np.asarray(obj_svd["center"]) - 1.0) * beta + 1.0, np.asarray(obj_svd["scale"]) * beta,
                              obj_svd["v"], obj_svd["d"])
    return dict(obj_svd_ref=obj_svd, simple_proj=XV, OADP_proj=oadp)
