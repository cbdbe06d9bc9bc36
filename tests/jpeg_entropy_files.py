"""Files shared by tests/test_jpeg_entropy_cpu.py and tests/test_gpu_jpeg_entropy.py besides those of tests/jpeg_files.py:
three hand-made damaged files.  The CPU test runs each through the host twin of the device decoder under the sanitizers and
asserts what is said about it here; the GPU test then decodes the same bytes on the device."""
import jpeg_files as J


def scan_start(data: bytes) -> int:
    """offset of the first entropy-coded byte"""
    sos = J._sos(data)
    return sos + 1 + 2 * data[sos] + 3


def base() -> bytes:
    return J.plain(64, 48, 2, False, 85)


def truncated() -> bytes:
    """cut 300 bytes into the scan: the host decoder reads zeros from there on and still gives a picture"""
    data = base()
    return data[:scan_start(data) + 300]


def flipped() -> bytes:
    """one bit of one scan byte changed: another valid picture for the host decoder"""
    data = bytearray(base())
    data[scan_start(data) + 40] ^= 0x10
    return bytes(data)


def bad_code() -> bytes:
    """32 one bits in the scan (FF 00 four times): no code of the standard tables is all ones, so the host decoder refuses
    the file with "bad Huffman code in JPEG data" """
    data = bytearray(base())
    at = scan_start(data) + 40
    data[at:at + 8] = b"\xff\x00" * 4
    return bytes(data)


DAMAGED = [("truncated", truncated, True), ("flipped", flipped, True), ("bad-code", bad_code, False)]   # name, maker, host accepts


def sequential_files():
    return [(name, make) for name, make in J.FILES if "-prog-" not in name]


def progressive_files():
    return [(name, make) for name, make in J.FILES if "-prog-" in name]
