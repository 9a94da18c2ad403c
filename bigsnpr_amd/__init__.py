"""bigsnpr_amd — MI355X (gfx950) implementation of bigsnpr's genotype-matrix hot path.

The product is libbigsnpr_hip.so (hand-written HIP kernels behind the C ABI of
include/bigsnpr_hip.h); this package is the host-side mirror of the reference's R API
used by the tests and the benchmark.  No CPU fallback exists anywhere in this package.
"""
from ._lib import BsnError, DeviceArray, load  # noqa: F401
from .bed import (ERROR_DIM, ScaledOp, bed, bed_colstats, bed_counts, bed_cprodVec,  # noqa: F401
                  bed_MAF, bed_prodVec, bed_scaleBinom, cols_along, read_bed,
                  read_bed_scaled, rows_along, sub_bed)
from .svd import bed_randomSVD  # noqa: F401,E402
from .comm import Comm, negotiate as negotiate_exchange, set_exchange_mode  # noqa: F401,E402
from .ld import (CODE_012, CODE_DOSAGE, CODE_IMPUTE_PRED, FBM_code256, bed_clumping, bed_cor,  # noqa: F401,E402
                 bed_ld_scores, big_cprodVec, big_prodVec, big_randomSVD, snp_clumping, snp_fake, snp_colstats, snp_cor, snp_ld_scores, snp_MAF, snp_scaleAlpha,
                 snp_scaleBinom)
from .prs import (bed_projectSelfPCA, bed_tcrossprodSelf, pca_OADP_proj2, pca_OADP_proj_device,  # noqa: F401,E402
                  prod_and_rowSumsSq, prod_and_rowSumsSq2, prodVecRev, project_pca, snp_PRS, snp_projectSelfPCA)
from .autosvd import bed_autoSVD, snp_autoSVD  # noqa: F401,E402
from .match import same_ref, snp_match  # noqa: F401,E402
from .project import bed_projectPCA  # noqa: F401,E402
from .plink_io import bed_to_bytes, snp_readBed, snp_writeBed  # noqa: F401,E402
from .pcadapt import bed_pcadapt, multLinReg, snp_pcadapt  # noqa: F401,E402
from .gwas import big_univLinReg, big_univLogReg  # noqa: F401,E402
from .impute import predictor_lists, snp_fastImpute, snp_fastImputeSimple  # noqa: F401,E402
from .bgen import check_bgen_format, format_snp_id, snp_prodBGEN, snp_readBGEN, snp_readBGI  # noqa: F401,E402
from .popstat import bed_counts_by_group, bed_fst, bed_MAF_by_group, snp_fst, snp_MAX3  # noqa: F401,E402
from .king import bed_king, bed_kingQC, king_last_ms, king_norel  # noqa: F401,E402
from .ibd import bed_ibd, bed_ibdQC, ibd_last_ms, indep_pairwise, prune_walk  # noqa: F401,E402
from .outliers import LOF, knn_last_stats, knn_parallel, lof_matrix, prob_dist, rob_maha  # noqa: F401,E402
from .ancestry import (AncestryProportions, ancestry_last_ms, ancestry_moments, bed_ancestry, nearPD, qp_simplex,  # noqa: F401,E402
                       snp_ancestry_summary)
from .scores import (AUC, AUCBoot, BootAUC, auc_boot_draws, auc_last_ms, big_prodMat, boot_statistics, pcor,  # noqa: F401,E402
                     snp_grid_AUC)
from .qc import bed_hwe, bed_plinkQC, bed_plinkRmSamples, hwe_exact_counts, qc_classes, qc_last_ms  # noqa: F401,E402
from .sct import seq_log, snp_grid_clumping, snp_grid_PRS, snp_grid_stacking  # noqa: F401,E402
from .plr import BigSpReg, big_spLinReg, big_spLogReg  # noqa: F401,E402
from .lassosum2 import SFBM, as_SFBM, snp_lassosum2  # noqa: F401,E402
from .ldsplit import snp_ldsplit  # noqa: F401,E402
from .ldpred2 import (coef_to_liab, ld_scores_sfbm, snp_ldpred2_auto, snp_ldpred2_grid, snp_ldpred2_inf,  # noqa: F401,E402
                      snp_ldsc, snp_ldsc2, sp_colSumsSq_sym, sp_cprodVec, sp_prodVec, sp_solve_sym)


def selftest():
    from ._lib import check
    check(load().bsn_selftest())


def device_count():
    import ctypes
    n = ctypes.c_int(0)
    load().bsn_device_count(ctypes.byref(n))
    return n.value
