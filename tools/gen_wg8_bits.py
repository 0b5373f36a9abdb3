#!/usr/bin/env python3
"""Write tests/golden/wg8_bits_fe_b.json: the digests tests/test_gpu_wg8_bits.py compares the 512-thread per-hop kernel with (needs a GPU).

    python tools/gen_wg8_bits.py [--out FILE] [--lib ab/lib_<tag>.so]

Run it on the commit whose bits are to be kept - the parent of a change that must not move them -, never on the change itself.  The runs
are the test's own (run_cases in tests/test_gpu_wg8_bits.py); --lib swaps in a side build (FE_BUILD_TAG) of that commit."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "wg8_bits_fe_b.json"))
    ap.add_argument("--lib", help="a side build's library instead of the in-tree one")
    a = ap.parse_args()
    if a.lib:
        os.environ["FASTENHANCER_HIP_LIB"] = os.path.abspath(a.lib)
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import test_gpu_wg8_bits as bits
    from fastenhancer_amd.build import source_key
    doc = bits.run_cases()
    doc["shape"] = bits.NAME
    doc["source_key"] = source_key() if not a.lib else None
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    for name, hops in doc["cases"].items():
        print(f"{name:<28}{hops[0]['kernel']}")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
