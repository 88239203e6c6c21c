"""enc_attention_x3_kernel (csrc/attention_x3.hip) over six to eight key steps - two and more turns of its three-slot ring,
every n_steps mod 3, odd and even tile counts, partial last tiles of 1 and 31 keys (tests/attn_x3_step_cases.py) - at d = 128,
H = 2, with plain pointers and with a table of three sessions, as fp32 rows and as an X3 result image.

Each launch goes through wlk_diag_enc_op with the guard words of tests/test_gpu_enc_x3.py and is judged like that file's
`attention` family: against the float64 reference, allowed 4 x the error of the float32 restatement on the same case
(enc_x3_reference.judge, family "attention_x3": no factor of its own).  The result must also be, bit for bit, what the kernel
wrote before its address arithmetic was taken out of the key loop: tests/golden/attn_x3_parent_bits.json holds a SHA-256 of
the result buffer per case, recorded by scripts/gen_golden_attn_x3_bits.py at that commit on an MI355X."""
import json
import os

import numpy as np
import pytest

import attn_x3_step_cases as SC
import enc_x3_reference as ER
import test_gpu_enc_x3 as TX

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", SC.GOLDEN)) as _fh:
    PARENT = json.load(_fh)["sha256"]


def test_the_golden_file_has_every_case():
    assert sorted(PARENT) == sorted(SC.key(T, b, x) for T in SC.GOLDEN_T for b in SC.BATCHES for x in (False, True))


@pytest.mark.parametrize("batch", SC.BATCHES)
@pytest.mark.parametrize("T", SC.GOLDEN_T)
def test_steps(T, batch):
    c = SC.case(T, batch)
    ref, f32 = ER.attention(c["qkv"], c["H"], np.float64), ER.attention(c["qkv"], c["H"], np.float32)
    failures, got = [], {}
    for x3_out in (False, True):
        tag = SC.key(T, batch, x3_out)
        call = TX.Attention(c, x3_out)
        assert call.rc == 0, call.msg
        failures += call.op.check_words(tag, {call.key: call.own})
        got[x3_out], canonical = call.values()
        entry, fail = ER.judge(tag, got[x3_out], ref, f32, "attention_x3")
        print(tag, c["inputs"], json.dumps(entry))
        failures += [fail] if fail else []
        if not canonical:
            failures.append(f"{tag}: the image is not the canonical split of float32 values")
        if SC.digest(call) != PARENT[tag]:
            failures.append(f"{tag}: the result's bits differ from the parent kernel's")
    if not np.array_equal(got[False], got[True]):
        failures.append(f"T={T} batch={batch}: the x3_out rows differ from the fp32 rows in {int((got[False] != got[True]).sum())} values")
    assert not failures, "\n".join(failures)
