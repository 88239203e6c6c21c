#!/usr/bin/env python
"""Records what enc_attention_x3_kernel writes, as one SHA-256 per case, into tests/golden/attn_x3_parent_bits.json.

Run it on an MI355X at the commit whose bits are to be kept (the parent of a change that must not move a bit); it uses
only wlk_diag_enc_op and the cases of tests/attn_x3_step_cases.py.  tests/test_gpu_attn_x3_steps.py compares the kernel of
the tree it runs in with the file.  GPU box only."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import attn_x3_step_cases as SC  # noqa: E402
import test_gpu_enc_x3 as TX  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", SC.GOLDEN)
    digests = {}
    for T in SC.GOLDEN_T:
        for batch in SC.BATCHES:
            c = SC.case(T, batch)
            for x3_out in (False, True):
                call = TX.Attention(c, x3_out)
                assert call.rc == 0, call.msg
                again = TX.Attention(c, x3_out)
                assert again.rc == 0 and SC.digest(again) == SC.digest(call), f"{c['name']}: two launches differ"
                digests[SC.key(T, batch, x3_out)] = SC.digest(call)
                print(SC.key(T, batch, x3_out), digests[SC.key(T, batch, x3_out)], flush=True)
    with open(out, "w") as fh:
        json.dump(dict(kernel="enc_attention_x3_kernel", d=SC.D, n_head=SC.H, sha256=digests), fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(f"wrote {out}: {len(digests)} digests")


if __name__ == "__main__":
    main()
