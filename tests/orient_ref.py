"""apply_orientation of host/image_io.cpp (image_io.hpp:39-41) restated on arrays, for tests/jpeg_files.py and
tests/png_files.py.  tests/test_jpeg_cpu.py and tests/test_png_decode_cpu.py hold it to host_selftest's output."""
import numpy as np


def orient(img: np.ndarray, orientation: int) -> np.ndarray:
    if orientation == 2:
        return img[:, ::-1]
    if orientation == 3:
        return img[::-1, ::-1]
    if orientation == 4:
        return img[::-1]
    if orientation == 5:
        return img.transpose(1, 0, 2)
    if orientation == 6:
        return img[::-1].transpose(1, 0, 2)
    if orientation == 7:
        return img[::-1, ::-1].transpose(1, 0, 2)
    if orientation == 8:
        return img[:, ::-1].transpose(1, 0, 2)
    return img
