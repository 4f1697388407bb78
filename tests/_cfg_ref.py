"""Numpy reference of the conditioning-dropout draw (vdm_cond_keep), in the conventions of tests/_philox_ref.py:

  consumer                     key                    counter (c0, c1, c2, c3)              use of the four words
  cond_keep(seed, p)           mix_seed(seed, step)   (row lo, row hi, 0xCFD0, 0)           keep = unit(word 0) > float32(p)

row = row0 + r is the GLOBAL row (rank * B + i): a row's fate depends neither on the rank layout nor on how many rows are drawn."""
import numpy as np

from _philox_ref import mix_seed, stream_words, unit

SID_COND_KEEP = 0xCFD0


def keep_rows(seed, p, row0, rows, step=None):
    """float32 [rows] of {0, 1}: what vdm_cond_keep(p, seed, seed_step -> step, row0, rows) writes."""
    idx = np.uint64(int(row0)) + np.arange(rows, dtype=np.uint64)
    w = stream_words(mix_seed(seed, step), SID_COND_KEEP, idx)
    return (unit(w[0]) > np.float64(np.float32(p))).astype(np.float32)
