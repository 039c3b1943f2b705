"""Write tests/golden/g15_pil_resize.npz: Pillow's own Image.resize(size, resample=Image.BILINEAR) on small 8-bit grey
images, the yardstick tests/_resize_ref.py (and through it K21, az_resample.hip) is held against where Pillow is not
installed.  Needs Pillow and no GPU.

    python tools/make_resize_goldens.py [--check]

Per case i of tests/_resize_ref.py GOLDEN_CASES: in_rand_i / out_rand_i (a seeded random image) and in_bin_i / out_bin_i
(a 0 / 255 image); stripes_in / stripes_out: the 1 x 8 image 0, 255, ... -> 1 x 6; sizes [cases, 4] = Hin, Win, Hout, Wout;
pil_version: PIL.__version__ of the run that wrote the file.  --check compares instead of writing."""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from tests import _resize_ref as ref  # noqa: E402

PATH = os.path.join(REPO, "tests", "golden", "g15_pil_resize.npz")


def pil_resize(img, size):
    from PIL import Image

    return np.array(Image.fromarray(img, mode="L").resize((size[1], size[0]), resample=Image.BILINEAR))


def arrays():
    import PIL

    out = {"pil_version": np.array(PIL.__version__), "stripes_in": ref.STRIPES,
           "stripes_out": pil_resize(ref.STRIPES, (1, 6)),
           "sizes": np.array([[*a, *b] for a, b in ref.GOLDEN_CASES], np.int32)}
    for i, ((hin, win), size) in enumerate(ref.GOLDEN_CASES):
        for kind, binary in (("rand", False), ("bin", True)):
            img = ref.make_image(i, hin, win, binary)
            out[f"in_{kind}_{i}"], out[f"out_{kind}_{i}"] = img, pil_resize(img, size)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="compare with the committed file instead of writing it")
    args = ap.parse_args()
    new = arrays()
    if args.check:
        old = np.load(PATH)
        bad = [k for k in new if k != "pil_version" and not np.array_equal(old[k], new[k])]
        print(f"Pillow {new['pil_version']} against the file written with {old['pil_version']}: "
              f"{len(bad)} of {len(new) - 1} arrays differ {bad}")
        return 1 if bad else 0
    np.savez_compressed(PATH, **new)
    print(f"wrote {PATH} ({os.path.getsize(PATH)} bytes) with Pillow {new['pil_version']}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
