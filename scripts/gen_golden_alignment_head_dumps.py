#!/usr/bin/env python
"""tests/golden/alignment_head_dumps.json: the reference's base85+gzip alignment-head masks
(whisperlivekit/whisper/__init__.py:39-54) as they stand there, name -> dump string; their decoded pairs are
tests/golden/alignment_heads.json (gen_golden_alignment_heads.py).
Build container only:  python scripts/gen_golden_alignment_head_dumps.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_stubs  # noqa: E402

ref_stubs.install()
import whisperlivekit.whisper as W  # noqa: E402

out = {name: dump.decode("ascii") for name, dump in W._ALIGNMENT_HEADS.items()}
json.dump(out, open(os.path.join(os.path.dirname(HERE), "tests", "golden", "alignment_head_dumps.json"), "w"), indent=0)
print(sorted(out))
