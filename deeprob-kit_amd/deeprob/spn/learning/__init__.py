from .em import expectation_maximization
from .learnspn import learn_spn
from .wrappers import learn_estimator, learn_classifier, compute_data_domains
from .cnet_bayesian import learn_cnet_bd, learn_cnet_bic
from .xpc import learn_xpc, learn_expc, SD_LEVEL_0, SD_LEVEL_1, SD_LEVEL_2, SD_LEVELS
