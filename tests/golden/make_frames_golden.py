"""Writes tests/golden/frames_resize.npz: the small cases of tests/_frames_cases.py with Pillow's own output for every filter, so
that the definition `frames._resize_u8_host` is held to does not drift with the Pillow build of another machine.  Uses PIL only.

    python tests/golden/make_frames_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _frames_cases as FC  # noqa: E402


def main():
    import PIL
    data = {"pillow_version": np.array(PIL.__version__)}
    for name, (H, W), (oh, ow) in FC.SMALL:
        a = FC.image(name, H, W, C=1)            # one channel: the channels are independent
        data[f"{name}/in"] = a
        for flt in FC.FILTERS:
            data[f"{name}/{flt}"] = FC.pillow_resize(a, (oh, ow), flt)
    path = os.path.join(HERE, "frames_resize.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
