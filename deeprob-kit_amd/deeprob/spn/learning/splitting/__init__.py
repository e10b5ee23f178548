"""The splitting methods of the reference (deeprob/spn/learning/splitting) that exist as functions on the HIP path: the RDC
split (``rdc_cols``, ``rdc_scores``), the entropy and Gini splits and the G-test splits.  ``learn_spn`` takes each of the
``*_cols`` functions as ``split_cols``, recognised by identity; the other methods are reached through its names.  The row clusterings ``gmm`` and ``kmeans`` (cluster.py) are functions
to call on their own and, by identity, ``split_rows`` of ``learn_spn``; ``split_rows_clusters`` (rows.py) is the reference's
host function."""
from .rdc import rdc_cols, rdc_scores
from .entropy import entropy_cols, entropy_adaptive_cols
from .gini import gini_cols, gini_adaptive_cols
from .gvs import gvs_cols, rgvs_cols, gtest
from .cluster import gmm, kmeans
from .rows import split_rows_clusters
