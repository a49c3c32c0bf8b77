#!/usr/bin/env python
"""sha256 of the device code inside a built library (no GPU needed): for every
gfx950 code object (one per translation unit, in link order) the digests of its
.text, .rodata and .note sections.  Two builds whose digests agree run the same
kernels with the same resources; whole-file hashes differ even then (the
__hip_cuid_* symbol is named after a hash of the source file).

  python3 tools/device_sections.py adversarial-collaborative-filtering_amd/lib/libacf_apr.so
  python3 tools/device_sections.py --compare tools/libacf_apr_<rev>.so <lib> [out.json]

--compare prints (and writes) both outputs and whether every digest is equal.
"""
from __future__ import annotations

import hashlib
import json
import os
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_resources import LLVM, code_objects  # noqa: E402

SECTIONS = (".text", ".rodata", ".note")


def digests(lib: str) -> list[dict]:
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        for co in code_objects(lib):
            path = os.path.join(tmp, "co")
            with open(path, "wb") as f:
                f.write(co)
            entry = {}
            for sec in SECTIONS:
                dump = os.path.join(tmp, "sec")
                subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", f"--only-section={sec}",
                                path, dump], check=True)
                with open(dump, "rb") as f:
                    data = f.read()
                entry[sec] = {"bytes": len(data), "sha256": hashlib.sha256(data).hexdigest()}
            out.append(entry)
    return out


def main(argv: list[str]) -> int:
    if argv and argv[0] == "--compare":
        base, new = digests(argv[1]), digests(argv[2])
        res = {"base": {"lib": argv[1], "code_objects": base}, "new": {"lib": argv[2], "code_objects": new},
               "all_equal": len(base) > 0 and base == new}
        text = json.dumps(res, indent=1)
        print(text)
        if len(argv) > 3:
            with open(argv[3], "w") as f:
                f.write(text + "\n")
        return 0 if res["all_equal"] else 1
    for k, entry in enumerate(digests(argv[0])):
        for sec in SECTIONS:
            print(k, sec, entry[sec]["bytes"], entry[sec]["sha256"])
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
