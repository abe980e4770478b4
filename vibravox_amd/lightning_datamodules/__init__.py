from .local_bwe import LocalBWEDataModule
from .local_noisybwe import LocalNoisyBWEDataModule

__all__ = ["LocalBWEDataModule", "LocalNoisyBWEDataModule"]
