from .classic import BatchedCartPole, BatchedPendulum
from .synthetic import BatchedSyntheticEnv, make_env

__all__ = ["BatchedCartPole", "BatchedPendulum", "BatchedSyntheticEnv",
           "make_env"]
