"""Write tests/golden/g16_result_images.npz and activezero_amd/csrc/az_viridis_table.h: matplotlib's own plt.imsave on the
small cases of tests/_result_images_ref.py, the yardstick that restatement (and through it K24, az_result_img.hip) is held
against where matplotlib is not installed.  Needs matplotlib and Pillow, and no GPU.

    python tools/make_result_image_goldens.py [--check]

plt.imsave is called as the reference's utils/test_util.py:59-107 save_img calls it -- a viridis copy with set_bad("red"),
np.ma.masked_where(x == -1, x), vmin=0, vmax=max_disp or 1.25; the two error images without a colour map -- into an
in-memory PNG that is decoded again, on the arrays test.py:235-260 hands it: the four float maps with [~mask] = -1 and the
two error images of tests/_gt_prep_ref.error_img.  One image at a time: the reference has no batch.

Per case NAME of ref.build_cases(): NAME/pred (the stored prediction, padded where the case is pitched), NAME/view (first row,
H, W of the view into it), NAME/gt_disp, NAME/gt_depth, NAME/mask, NAME/focal, NAME/baseline (per image), NAME/max_disp,
NAME/images uint8 [B,6,H,W,4]; viridis_table uint8 [256,3]: (lut * 255).astype(uint8) of the colour map; mpl_version.
--check compares instead of writing."""
import argparse
import io
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from tests import _gt_prep_ref as G  # noqa: E402
from tests import _result_images_ref as ref  # noqa: E402

PATH = os.path.join(REPO, "tests", "golden", "g16_result_images.npz")
HEADER = os.path.join(REPO, "activezero_amd", "csrc", "az_viridis_table.h")


def viridis_table():
    import matplotlib.pyplot as plt

    cmap = plt.get_cmap("viridis")
    table = cmap(np.arange(256), bytes=True)  # integers index the table: (lut * 255).astype(uint8) row by row
    assert table.dtype == np.uint8 and table.shape == (256, 4) and (table[:, 3] == 255).all()
    return np.ascontiguousarray(table[:, :3])


def header_text(table):
    rows = [", ".join("{%d, %d, %d}" % tuple(int(c) for c in rgb) for rgb in table[i:i + 8]) for i in range(0, 256, 8)]
    return ("// matplotlib's viridis as bytes: (lut * 255).astype(uint8) of plt.get_cmap(\"viridis\"), 256 rows R, G, B; alpha is\n"
            "// 255.  DATA: written and compared by tools/make_result_image_goldens.py, never edited by hand.\n"
            "#pragma once\n"
            "static __constant__ unsigned char az_viridis_rgb[256][3] = {\n    " + ",\n    ".join(rows) + "};\n")


def imsave_bytes(arr, **kw):
    import matplotlib.pyplot as plt
    from PIL import Image

    buf = io.BytesIO()
    plt.imsave(buf, arr, format="png", **kw)
    buf.seek(0)
    img = Image.open(buf)
    assert img.mode == "RGBA"
    return np.array(img)


def save_img_panels(pred_disp, gt_disp, gt_depth, mask, fb, max_disp):
    """uint8 [6,H,W,4]: what test.py:235-272 writes for ONE image ([H,W] float32 maps, bool mask, fb float32)"""
    import matplotlib.pyplot as plt

    cmap = plt.get_cmap("viridis").copy()
    cmap.set_bad(color="red")
    with np.errstate(all="ignore"):
        pred_depth = np.float32(fb) / pred_disp  # test.py:209 (the product is the caller's)
        err_disp = G.error_img(pred_disp[None], gt_disp[None], mask[None], "disp")[0]  # test.py:244
        err_depth = G.error_img((pred_depth * np.float32(1000))[None], (gt_depth * np.float32(1000))[None], mask[None],
                                "depth")[0]  # test.py:260
    panels = {}
    for m, (x, vmax) in {0: (pred_disp, max_disp), 1: (gt_disp, max_disp), 3: (pred_depth, 1.25), 4: (gt_depth, 1.25)}.items():
        x = x.copy()
        x[~mask] = -1
        with np.errstate(all="ignore"):
            panels[m] = imsave_bytes(np.ma.masked_where(x == -1, x), cmap=cmap, vmin=0, vmax=vmax)
    panels[2], panels[5] = imsave_bytes(err_disp), imsave_bytes(err_depth)
    plt.close("all")
    return np.stack([panels[m] for m in range(6)])


def matplotlib_images(case):
    """uint8 [B,6,H,W,4] of a case of tests/_result_images_ref.py, image by image"""
    pred = ref.pred_view(case)
    md = case["max_disp"]
    md = int(md) if float(md).is_integer() else float(md)  # cfg.MODEL.MAX_DISP is an int
    return np.stack([save_img_panels(pred[b, 0].copy(), case["gt_disp"][b, 0], case["gt_depth"][b, 0],
                                     case["mask"][b, 0].astype(bool), np.float32(case["focal"][b]) * np.float32(case["baseline"][b]),
                                     md) for b in range(pred.shape[0])])


def arrays():
    import matplotlib

    out = {"mpl_version": np.array(matplotlib.__version__), "viridis_table": viridis_table()}
    for name, case in ref.build_cases().items():
        for k in ref.INPUTS:
            out[f"{name}/{k}"] = np.asarray(case[k])
        out[f"{name}/images"] = matplotlib_images(case)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="compare with the committed files instead of writing them")
    args = ap.parse_args()
    new = arrays()
    text = header_text(new["viridis_table"])
    if args.check:
        old = np.load(PATH)
        bad = [k for k in new if k != "mpl_version" and not (k in old and np.array_equal(old[k], new[k], equal_nan=old[k].dtype.kind == "f"))]
        bad += [k for k in old.files if k not in new]
        with open(HEADER) as f:
            if f.read() != text:
                bad.append(os.path.basename(HEADER))
        print(f"matplotlib {new['mpl_version']} against the files written with {old['mpl_version']}: "
              f"{len(bad)} of {len(new)} differ {bad}")
        return 1 if bad else 0
    np.savez_compressed(PATH, **new)
    with open(HEADER, "w") as f:
        f.write(text)
    print(f"wrote {PATH} ({os.path.getsize(PATH)} bytes) and {HEADER} with matplotlib {new['mpl_version']}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
