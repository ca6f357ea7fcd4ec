"""ctypes access to oracle/_ref/libstb_ref.so = the reference's vendored
stb_image v2.27 + stb_image_write v1.16 compiled from /root/reference/vendor by
oracle/Makefile.  Test infrastructure only.  Where that build is absent, `recorded()`
stands in for it: what the build returned for every input the tests hand it, as shape +
SHA-256 of each decoded image and length + SHA-256 of each PNG file
(tests/golden/stb_recorded.json; add to it where the build exists with
HMRM_STB_RECORD=tests/golden/stb_recorded.json pytest tests/test_image_io.py).  Only
what the tests compare is asked for, and so recorded: stb answers some refused inputs
from uninitialised memory."""
import atexit
import ctypes as C
import hashlib
import json
import os

import numpy as np

_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", "libstb_ref.so")
_RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stb_recorded.json")


def _sha(data) -> str:
    return hashlib.sha256(data).hexdigest()


def _load_key(data: bytes, req_comp: int) -> str:
    return f"load {_sha(data)} {req_comp}"


def _png_key(img: np.ndarray) -> str:
    img = np.ascontiguousarray(img, dtype=np.uint8)
    return f"png {'x'.join(map(str, img.shape))} {_sha(img.tobytes())}"


def _array_digest(arr: np.ndarray):
    return {"shape": list(arr.shape), "sha256": _sha(np.ascontiguousarray(arr).tobytes())}


class StbRef:
    def __init__(self, lib):
        self.lib = lib
        lib.stbi_load_from_memory.restype = C.POINTER(C.c_uint8)
        lib.stbi_load_from_memory.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                              C.POINTER(C.c_int), C.c_int]
        lib.stbi_image_free.argtypes = [C.c_void_p]
        lib.stbi_write_png_to_mem.restype = C.POINTER(C.c_uint8)
        lib.stbi_write_png_to_mem.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
        lib.stbi_failure_reason.restype = C.c_char_p

    def load(self, data: bytes, req_comp: int):
        """-> (array HxWxC, channels_in_file) or (None, reason)."""
        x, y, n = C.c_int(), C.c_int(), C.c_int()
        p = self.lib.stbi_load_from_memory(data, len(data), C.byref(x), C.byref(y), C.byref(n), req_comp)
        if not p:
            return None, (self.lib.stbi_failure_reason() or b"").decode()
        comp = req_comp if req_comp else n.value
        arr = np.ctypeslib.as_array(p, shape=(y.value, x.value, comp)).copy()
        self.lib.stbi_image_free(p)
        return arr, n.value

    def write_png(self, img: np.ndarray) -> bytes:
        img = np.ascontiguousarray(img, dtype=np.uint8)
        h, w, comp = img.shape
        n = C.c_int()
        p = self.lib.stbi_write_png_to_mem(img.ctypes.data, w * comp, w, h, comp, C.byref(n))
        data = bytes(np.ctypeslib.as_array(p, shape=(n.value,)))
        libc = C.CDLL(None)
        libc.free.argtypes = [C.c_void_p]
        libc.free(p)
        return data

    @staticmethod
    def same(arr: np.ndarray, exp: np.ndarray) -> bool:
        return np.array_equal(arr, exp)


class Digest:
    """A recorded stb result: a decoded image (shape + SHA-256 of its uint8 samples) or a PNG file (length + SHA-256)."""

    def __init__(self, sha256, shape=None, length=None):
        self.sha256, self.shape, self.length = sha256, shape, length

    def __eq__(self, other):
        if isinstance(other, (bytes, bytearray)):
            return self.length == len(other) and self.sha256 == _sha(other)
        other = np.asarray(other)
        return (other.dtype == np.uint8 and self.shape == list(other.shape)
                and self.sha256 == _sha(np.ascontiguousarray(other).tobytes()))

    __hash__ = None


class RecordedStb:
    """Answers like StbRef from tests/golden/stb_recorded.json; an input the record does not hold is an error."""

    def __init__(self, path=_RECORD):
        with open(path) as f:
            self.rec = json.load(f)

    def _get(self, key):
        if key not in self.rec:
            raise KeyError(f"{key}: not among the recorded results of the reference's stb ({_RECORD}); "
                           "record it where oracle/_ref is built (see tests/stb_ref.py)")
        return self.rec[key]

    def load(self, data: bytes, req_comp: int):
        e = self._get(_load_key(data, req_comp))
        if "reason" in e:
            return None, e["reason"]
        return Digest(e["sha256"], shape=e["shape"]), e["n"]

    def write_png(self, img: np.ndarray):
        e = self._get(_png_key(img))
        return Digest(e["sha256"], length=e["length"])

    @staticmethod
    def same(arr: np.ndarray, exp: Digest) -> bool:
        return exp == arr


class RecordingStb(StbRef):
    """The live build, writing every answer it gives into the record at exit (HMRM_STB_RECORD=<path>)."""

    def __init__(self, lib, path):
        super().__init__(lib)
        self.path, self.rec = path, {}
        atexit.register(self.save)

    def load(self, data: bytes, req_comp: int):
        arr, n = super().load(data, req_comp)
        self.rec[_load_key(data, req_comp)] = {"reason": n} if arr is None else dict(_array_digest(arr), n=n)
        return arr, n

    def write_png(self, img: np.ndarray) -> bytes:
        data = super().write_png(img)
        self.rec[_png_key(img)] = {"length": len(data), "sha256": _sha(data)}
        return data

    def save(self):
        """Merged into the record already at `path` (a run of some of the tests keeps the others' entries); delete the
        file first to rebuild it from what the tests ask now."""
        rec = {}
        if os.path.exists(self.path):
            with open(self.path) as f:
                rec = json.load(f)
        rec.update(self.rec)
        with open(self.path, "w") as f:  # (one entry per line)
            f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in sorted(rec.items())) + "\n}\n")


def load():
    """The live build, or None where it was never built."""
    if not os.path.exists(_PATH):
        return None
    if os.environ.get("HMRM_STB_RECORD"):
        return RecordingStb(C.CDLL(_PATH), os.environ["HMRM_STB_RECORD"])
    return StbRef(C.CDLL(_PATH))


def recorded():
    return RecordedStb()
