from .classic import (BatchedAcrobot, BatchedCartPole, BatchedCartPoleV1,
                      BatchedMountainCar, BatchedMountainCarContinuous,
                      BatchedPendulum)
from .synthetic import BatchedSyntheticEnv, make_env

__all__ = ["BatchedAcrobot", "BatchedCartPole", "BatchedCartPoleV1",
           "BatchedMountainCar", "BatchedMountainCarContinuous",
           "BatchedPendulum", "BatchedSyntheticEnv", "make_env"]
