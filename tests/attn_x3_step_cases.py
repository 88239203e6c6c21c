"""Cases that walk the three-slot ring of enc_attention_x3_kernel (csrc/attention_x3.hip) for six to eight key steps, and the
digest of a launch's result.  Shared by tests/test_gpu_attn_x3_steps.py and scripts/gen_golden_attn_x3_bits.py, so that the
test and the recorded bits of the parent kernel come from the same seeded inputs through the same diagnostic entry
(wlk_diag_enc_op, kind ENC_ATTENTION, with the guard words of tests/test_gpu_enc_x3.py).

T = 321 .. 512 is 11 .. 16 key tiles of 32, 6 .. 8 steps of two tiles: every n_steps mod 3, odd and even tile counts (an odd
count leaves the second stream without a last tile), partial last tiles of 1 key (321, 385, 449) and of 31 keys (447).
97 and 193 are the largest shapes of tests/enc_x3_cases.py, kept for the recorded bits."""
import hashlib
import zlib

import numpy as np

import enc_x3_cases as EC

STEP_T = (321, 352, 384, 385, 447, 449, 512)
GOLDEN_T = STEP_T + (97, 193)
D, H = 128, 2
BATCHES = (0, 3)
GOLDEN = "attn_x3_parent_bits.json"


def key(T, batch, x3_out):
    return f"t{T}_b{batch}_{'x3' if x3_out else 'fp32'}"


def case(T, batch):
    """-> an attention case in the form of enc_x3_cases.case: seeded by its name, the input kinds dealt round"""
    name = f"axs_t{T}_b{batch}"
    inputs = EC.ATT_KINDS[(GOLDEN_T.index(T) + (1 if batch else 0)) % len(EC.ATT_KINDS)]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    return dict(kind="attention", form=1, T=T, H=H, d=D, batch=batch, inputs=inputs, name=name,
                qkv=EC._qkv(rng, inputs, max(batch, 1), T, H))


def digest(call):
    """SHA-256 of the whole result buffer of a test_gpu_enc_x3.Attention call: the owned words and the guards around them"""
    return hashlib.sha256(np.ascontiguousarray(call.result).tobytes()).hexdigest()
