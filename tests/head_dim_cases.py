"""The two small decoder configurations of the head-dim training tests (tests/test_train_head_dims_gpu.py) and their
tolerances: R.TINY widened to a hidden size of 256 with 4 heads / 2 kv heads (head dim 64, grouped-query attention) and
2 heads / 1 kv head (head dim 128).  The tolerances are measured the way every model-level tolerance of the suite is
(2 x the error of stock bf16 ops on the same inputs, scripts/calibrate_tolerances.py --head-dims) and read from
tests/golden/tolerance_calibration_head_dims.json."""
import dataclasses
import json
import os

from oracle import restate as R

CONFIGS = {
    64: dataclasses.replace(R.TINY, hidden_size=256, num_attention_heads=4, num_key_value_heads=2),
    128: dataclasses.replace(R.TINY, hidden_size=256, num_attention_heads=2, num_key_value_heads=1),
}
assert all(cfg.head_dim == hd for hd, cfg in CONFIGS.items())
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tolerance_calibration_head_dims.json")
_TOL = None


def tol(hd: int, quantity: str) -> float:
    global _TOL
    if _TOL is None:
        _TOL = json.load(open(PATH))["quantities"]
    return float(_TOL[f"hd{hd}.{quantity}"]["tolerance"])
