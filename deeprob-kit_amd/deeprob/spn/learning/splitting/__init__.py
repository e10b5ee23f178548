"""The splitting methods of the reference (deeprob/spn/learning/splitting) that exist as functions on the HIP path.
Only ``rdc_cols`` and ``rdc_scores`` are built; the other methods are reached through ``learn_spn``'s names."""
from .rdc import rdc_cols, rdc_scores
