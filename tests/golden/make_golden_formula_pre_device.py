#!/usr/bin/env python3
"""Fixtures of the device formula pre-process, minted on the CPU with Pillow through rapiddoc_amd.formula_host.decode_image /
to_network_input (which tests/golden/formula_pre.json pins to the reference's own PPPreProcess).

    python tests/golden/make_golden_formula_pre_device.py      # writes tests/golden/formula_pre_device.json + formula_pre_device*.npz

Per crop (tests/formula_pre_reference.make_crop: a light patch with dark strokes in a sub-rectangle, regenerated from its seed and held
to a crc32): the margin box, the route the plan arithmetic gives it, the uint8 384 x 384 x 3 image and the crc32 of the float32 network
input.  The box sizes are asserted on the host result alone.  Every .npz stays below 1 MiB."""
import json
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parents[1]))
sys.path.insert(0, str(HERE.parent))

import formula_pre_reference as R                      # noqa: E402
from rapiddoc_amd import formula_host as FH            # noqa: E402

LIMIT = 1 << 20


def main():
    cases, arrays = [], {}
    for seed, box_hw in enumerate(R.BOX_SIZES):
        crop = R.make_crop(seed, box_hw)
        pil = FH._crop_margin(FH.Image.fromarray(crop).convert("RGB"))           # the host's own box: its size is what the table asks for
        want = box_hw if box_hw is not None else R.UNIFORM_HW
        assert (pil.height, pil.width) == tuple(want), (seed, box_hw, pil.size)
        box = R.margin_box(crop)
        assert (box[3] - box[1], box[2] - box[0]) == tuple(want)
        assert np.array_equal(np.asarray(pil), crop[box[1]: box[3], box[0]: box[2]])
        route = "device" if R.plan(box[2] - box[0], box[3] - box[1])["served"] else "host"
        assert (route == "host") == (box_hw in R.HOST_ROUTE_BOXES), (box_hw, route)
        u8 = FH.decode_image(crop)
        x = FH.to_network_input(u8)
        assert u8.shape == (384, 384, 3) and x.shape == (1, 1, 384, 384) and x.dtype == np.float32
        name = "uniform" if box_hw is None else f"box_{box_hw[0]}x{box_hw[1]}"
        cases.append({"name": name, "seed": seed, "box_hw": list(box_hw) if box_hw else None, "crop_hw": list(crop.shape[:2]), "crop_crc32": R.crc(crop),
                      "box": list(box), "route": route, "u8_crc32": R.crc(u8), "input_crc32": R.crc(x)})
        arrays[f"u8_{seed}"] = u8
        print(name, crop.shape, box, route)
    for old in HERE.glob("formula_pre_device*.npz"):
        old.unlink()
    files, cur = [], {}

    def flush():
        if cur:
            path = HERE / f"formula_pre_device_{len(files)}.npz"
            np.savez_compressed(path, **cur)
            assert path.stat().st_size <= LIMIT, path
            files.append(path.name)
            cur.clear()

    import io
    size = 0
    for i, c in enumerate(cases):
        buf = io.BytesIO()
        np.savez_compressed(buf, a=arrays[f"u8_{i}"])
        if size + buf.tell() > LIMIT - 65536:
            flush()
            size = 0
        cur[f"u8_{i}"] = arrays[f"u8_{i}"]
        size += buf.tell()
        c["file"] = len(files)
    flush()
    (HERE / "formula_pre_device.json").write_text(json.dumps({"files": files, "cases": cases}, indent=1))
    print(files, [(HERE / f).stat().st_size for f in files])


if __name__ == "__main__":
    main()
