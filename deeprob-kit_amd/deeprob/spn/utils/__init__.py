"""Helpers of the structure learners (reference deeprob/spn/utils): ``partitioning``, the partition tree of an XPC."""
