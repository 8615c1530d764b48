#!/usr/bin/env python3
"""Regenerates kzg_trusted_setup_g2.bin (run where the reference checkout is at hand: `make_kzg_trusted_setup_g2.py REFERENCE_DIR`).

The 96 bytes of the hex string `setup_g2_1` is built from in the reference's kzg/src/lib.rs: the public ceremony output [tau] G2 as a
compressed G2 point (x.c1 then x.c0, big-endian, the flags in the first byte). Data only."""
import hashlib
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SHA256 = "4c495656b40ff5ae60187cbd968ce7999dfe53ca0364900338790d4c78f87114"

if __name__ == "__main__":
    text = open(os.path.join(sys.argv[1], "kzg", "src", "lib.rs")).read()
    block = text[text.index("let setup_g2_1"):]
    raw = bytes.fromhex(re.search(r'"([0-9a-f]{192})"', block).group(1))
    assert len(raw) == 96 and hashlib.sha256(raw).hexdigest() == SHA256
    open(os.path.join(HERE, "kzg_trusted_setup_g2.bin"), "wb").write(raw)
    print("ok", len(raw))
