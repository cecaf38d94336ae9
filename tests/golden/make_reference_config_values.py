"""Recorded flag values of the reference's own flagfiles -> tests/golden/reference_config_values.json.

    python tests/golden/make_reference_config_values.py --reference /path/to/symbolic-music-diffusion

Every ``configs/**/*.cfg`` of the reference (except the ``mdn-*`` flagfiles of train_mdn.py, a different flag set) is parsed by
``smd_amd.flags`` from the reference's root, as train_ncsn.py resolves nested ``--flagfile=configs/...`` lines, and the values of the flags
the file sets (directly or through nested flagfiles) are stored per file; every other flag keeps the parser's default.
tests/test_host.py compares the shipped ``configs/`` against these values.
"""
import argparse
import glob
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of magenta/symbolic-music-diffusion")
    ap.add_argument("--out", default=os.path.join(HERE, "reference_config_values.json"))
    a = ap.parse_args()
    import smd_amd.flags as F
    out = {}
    cwd = os.getcwd()
    os.chdir(a.reference)
    try:
        for f in sorted(glob.glob("configs/**/*.cfg", recursive=True)):
            if os.path.basename(f).startswith("mdn"):
                continue
            fl = F.make_flags(True)
            fl.parse([f"--flagfile={f}"])
            out[f] = {k: v for k, v in fl.flag_values_dict().items() if fl.is_present(k)}
    finally:
        os.chdir(cwd)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(f"{len(out)} flagfiles -> {a.out}")


if __name__ == "__main__":
    main()
