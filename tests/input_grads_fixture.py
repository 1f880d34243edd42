"""Reader of fixture F15 (tests/golden/make_golden_input_grads.py): the reference's float64 input gradients, stored as one small
archive plus numbered slices of the concatenated large arrays (no committed file may exceed 1 MiB)."""
import json

import numpy as np

from common import GOLDEN

_CACHE = {}


def load_f15():
    """{key: array}: the entries make_golden_input_grads.py documents, the g64:<mode>:<i> arrays reassembled"""
    if "f15" not in _CACHE:
        g = np.load(GOLDEN / "f15_input_grads.npz", allow_pickle=False)
        out = {k: g[k] for k in g.files}
        flat = np.concatenate([np.load(GOLDEN / f"f15_input_grads.part{k:02d}.npz", allow_pickle=False)["data"]
                               for k in range(int(g["nparts"]))])
        off = 0
        for name, shape in zip([str(k) for k in g["big_names"]], json.loads(str(g["big_shapes_json"]))):
            n = int(np.prod(shape))
            out[name] = flat[off:off + n].reshape(shape)
            off += n
        assert off == flat.size, "F15: the part files do not match the layout"
        _CACHE["f15"] = out
    return _CACHE["f15"]
