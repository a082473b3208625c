"""Layer tiling in numpy: the re-arrangement of include/piehip.h "Layer tiling", written once for the tests.

B = k*e slots per bin layer, R >= 1 bin layers per slot vector (R*B <= N), b' = ceil(b / R) tiled layers:
  tile_db_slots   slots'[h][g][j][r*B + s] = slots[h][g*R + r][j][s] for g*R + r < b, else 0
  tile_masks      mask'[g][r*B + s] = mask(layer g*R + r, slot s): the oracle's draw of b'*R layers, read as [b'][R*B]
  tile_vectors    the client's vectors, their B slots repeated R times
  untile          result row g, slots [r*B, (r+1)*B), is bin layer g*R + r; the blocks behind layer b - 1 are dropped
  unused_blocks   ... and those blocks themselves
"""
import numpy as np


def tiled_layers(b, R):
    return -(-b // R)


def tile_db_slots(slots, R):
    """[K][b][E][B] -> [K][b'][E][R*B]"""
    K, b, E, B = slots.shape
    bt = tiled_layers(b, R)
    padded = np.zeros((K, bt * R, E, B), dtype=slots.dtype)
    padded[:, :b] = slots
    return np.ascontiguousarray(padded.reshape(K, bt, R, E, B).transpose(0, 1, 3, 2, 4).reshape(K, bt, E, R * B))


def tile_masks(ob, t, b, B, seed, R):
    """[b'][R*B]"""
    bt = tiled_layers(b, R)
    return np.ascontiguousarray(ob.masks(t, bt * R, B, seed).reshape(bt, R * B))


def tile_vectors(vecs, R):
    """[..][B] -> [..][R*B]"""
    vecs = np.asarray(vecs)
    return np.ascontiguousarray(np.tile(vecs, (1,) * (vecs.ndim - 1) + (R,)))


def untile(rows, R, B, b):
    """decrypted result rows [b'][>= R*B] -> bin layers [b][B]"""
    rows = np.asarray(rows)
    return np.ascontiguousarray(rows[:, :R * B].reshape(rows.shape[0] * R, B)[:b])


def unused_blocks(rows, R, B, b):
    """the blocks of the last tiled layer that hold no bin layer, [b'*R - b][B]"""
    rows = np.asarray(rows)
    return rows[:, :R * B].reshape(rows.shape[0] * R, B)[b:]
