"""Fixed-width byte keys derived from an element's global index, shared by the byte-key element tests."""
import numpy as np


def _rows(ids, width):
    """width-byte key of element id: the splitmix stream of the id, little-endian words."""
    ids = np.asarray(ids, dtype=np.uint64)
    words = width // 8
    out = np.empty((ids.size, words), dtype=np.uint64)
    for w in range(words):
        z = ids * np.uint64(0x9E3779B97F4A7C15) + np.uint64((w * 0x632BE59BD9B4E019 + 1) & (2**64 - 1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        out[:, w] = z ^ (z >> np.uint64(31))
    return out.view(np.uint8).reshape(ids.size, width)


def _rows_at(writers, width):
    """The reservoir an oracle last-writer table stands for: _rows of each slot's writer, and
    `width` zero bytes where the slot has none (writer < 0)."""
    writers = np.asarray(writers, dtype=np.int64)
    out = np.zeros((writers.size, width), dtype=np.uint8)
    hit = writers >= 0
    out[hit] = _rows(writers[hit], width)
    return out
