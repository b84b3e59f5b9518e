"""tests/golden/ref_pattern_search_pu_wide.npz as the tests read it (test_oracle_golden_motion_pu_wide.py without a GPU, test_gpu_motion_pu_wide.py
on one): what the reference's own xPatternSearch returned at search ranges up to 64 for the 85 nodes, the 124 PUs and the 384 small PUs of five
CTUs of the ragged 176 x 144 picture (tests/quality/gen_motion_pu_wide_golden.py).  The layout and the reader are motion_golden's.  A plain
module, not a conftest."""
import motion_golden as mg

# valid entries per family as the generator printed them: 8 cases of 267 / 348 / 1224
WIDE_COUNTS = {"nodes": 2136, "pu": 2784, "small": 9792}
PER_CASE = {"nodes": 267, "pu": 348, "small": 1224}


def wide_cases():
    return mg._cases("ref_pattern_search_pu_wide.npz", mg.SearchCase, WIDE_COUNTS)
