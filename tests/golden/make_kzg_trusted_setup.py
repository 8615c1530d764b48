#!/usr/bin/env python3
"""Regenerates kzg_trusted_setup_g1.bin (run where the reference checkout is at hand: `make_kzg_trusted_setup.py REFERENCE_DIR`).

The 4 096 entries of the `g1_lagrange` list of the reference's kzg/src/trusted_setup.json, in file order, hex-decoded, 48 bytes each:
the public ceremony output (compressed G1 points [tau^k] G1; entry 0 is the generator). Data only."""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SHA256 = "08797579f6cfd5788eddc1a215d64dcfabd04acbcaf2953fb2c1afb830f43315"

if __name__ == "__main__":
    points = json.load(open(os.path.join(sys.argv[1], "kzg", "src", "trusted_setup.json")))["g1_lagrange"]
    raw = b"".join(bytes.fromhex(p[2:] if p.startswith("0x") else p) for p in points)
    assert len(raw) == 4096 * 48 and hashlib.sha256(raw).hexdigest() == SHA256
    open(os.path.join(HERE, "kzg_trusted_setup_g1.bin"), "wb").write(raw)
    print("ok", len(raw))
