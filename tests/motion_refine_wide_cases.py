"""tests/golden/ref_frac_search_wide.npz as the tests read it (test_oracle_golden_frac_wide.py without a GPU, test_gpu_motion_refine_pu_wide.py on
one): what the reference's own xPatternSearchFracDIF returned around integer vectors of up to +-64 samples for the 85 nodes, the 124 PUs and the
384 small PUs of five CTUs of the ragged 176 x 144 picture (tests/quality/gen_frac_search_wide_golden.py).  The layout and the reader are
motion_golden's.  A plain module, not a conftest."""
import motion_golden as mg

# valid entries per family as the generator printed them: 11 cases of 267 / 348 / 1224
WIDE_FRAC_COUNTS = {"nodes": 2937, "pu": 3828, "small": 13464}
PER_CASE = {"nodes": 267, "pu": 348, "small": 1224}


def wide_frac_cases():
    return mg._cases("ref_frac_search_wide.npz", mg.FracCase, WIDE_FRAC_COUNTS)
