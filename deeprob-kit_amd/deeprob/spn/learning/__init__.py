from .em import expectation_maximization
