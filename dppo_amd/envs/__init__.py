from .classic import BatchedAcrobot, BatchedCartPole, BatchedPendulum
from .synthetic import BatchedSyntheticEnv, make_env

__all__ = ["BatchedAcrobot", "BatchedCartPole", "BatchedPendulum",
           "BatchedSyntheticEnv", "make_env"]
