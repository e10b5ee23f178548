from .cltmix import BinaryCLTMixture
