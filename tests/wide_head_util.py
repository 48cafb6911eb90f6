"""The two reduced wide-head models shared by tests/test_wide_head_cpu.py (which pins the oracle to the Hugging Face classes
at these widths) and tests/test_wide_head_gpu.py (which compares the kernels with that oracle)."""
from eav_amd import synth
from tests.golden_util import tf_weights

# the two reduced wide-head configurations (shared with the GPU tests)
WIDE_CASES = {
    "ast": dict(hidden=64, layers=2, heads=4, ff=128, frames=128, num_labels=527),
    "vit": dict(hidden=64, layers=2, heads=4, ff=128, image=64, num_labels=1000),
}


def wide_case(kind, seed):
    """(oracle cfg, weights keyed by HF names) of a reduced wide-head model."""
    from oracle import vit_oracle as vo
    ocfg = (vo.cfg_ast if kind == "ast" else vo.cfg_vit)(**WIDE_CASES[kind])
    return ocfg, tf_weights(seed, vo.param_shapes(ocfg), std=0.05)


def wide_batch(kind, seed, B):
    c = WIDE_CASES[kind]
    return synth.mel_batch(seed, B, c["frames"], 128) if kind == "ast" else synth.frame_batch(seed, B, c["image"])
