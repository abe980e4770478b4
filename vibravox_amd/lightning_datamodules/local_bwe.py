"""``BWELightningDataModule`` (vibravox/lightning_datamodules/bwe.py:14-293) on recordings of one's own: the Hub source replaced by
``root/<subset>/<split>/<sensor>/<stem>.wav`` (``corpus.scan``), the splits resident in HBM (``corpus.ResidentCorpus``) and every batch
assembled on the device by ``collate.bwe_collate`` from views into the store.  ``sensor``, ``subset``, ``collate_strategy``,
``data_augmentation`` and ``batch_size`` keep the reference's meaning; ``shuffle`` (the reference's loader does not), ``drop_last``,
``device``, ``rank`` and ``world_size`` are additions."""
from __future__ import annotations

import re
from typing import Callable, Dict, List, Optional, Tuple

import torch

from .. import collate
from ..augment import WaveformDataAugmentation
from ..corpus import AIRBORNE, ResidentCorpus, epoch_plan


class ResidentLoader:
    """A re-iterable loader over the items of a resident split: every ``iter()`` is one epoch of ``corpus.epoch_plan`` (epochs count up
    from 0), every batch ``make_batch(indices)``."""

    def __init__(self, n_items: int, batch_size: int, make_batch: Callable[[List[int]], object], shuffle: bool = False, drop_last: bool = False,
                 seed: int = 0, rank: int = 0, world_size: int = 1):
        if batch_size < 1:
            raise ValueError(f"a loader's batch_size must be positive, got {batch_size}")
        self.n_items, self.batch_size, self.make_batch = n_items, batch_size, make_batch
        self.shuffle, self.drop_last, self.seed, self.rank, self.world_size = shuffle, drop_last, seed, rank, world_size
        self.epoch = 0

    def plan(self, epoch: int) -> List[List[int]]:
        return epoch_plan(self.n_items, self.batch_size, shuffle=self.shuffle, drop_last=self.drop_last, seed=self.seed, epoch=epoch, rank=self.rank,
                          world_size=self.world_size)

    def __len__(self) -> int:
        return len(self.plan(0))   # the count does not depend on the epoch's order

    def __iter__(self):
        plan = self.plan(self.epoch)
        self.epoch += 1
        for indices in plan:
            yield self.make_batch(indices)


class LocalBWEDataModule:
    def __init__(self, sample_rate: int = 16000, root: Optional[str] = None, root_secondary: Optional[str] = None, subset: str = "speech_clean",
                 sensor: str = AIRBORNE, collate_strategy: str = "constant_length-2500-ms", data_augmentation: Optional[torch.nn.Module] = None,
                 batch_size: int = 32, shuffle: bool = False, drop_last: bool = False, device="cuda", rank: int = 0, world_size: int = 1, seed: int = 0,
                 max_stage_bytes: int = 1 << 30, **kwargs):
        if root is None:
            raise ValueError("LocalBWEDataModule needs root: the directory holding <subset>/<split>/<sensor>/<stem>.wav")
        assert collate_strategy == "pad" or re.match(r"constant_length-\d+-ms", collate_strategy), \
            "collate_strategy must be 'pad' or match the pattern 'constant_length-XXX-ms'"
        if data_augmentation is None:
            data_augmentation = WaveformDataAugmentation(sample_rate)
        assert isinstance(data_augmentation, WaveformDataAugmentation), "data_augmentation must be a WaveformDataAugmentation"
        self.sample_rate, self.root, self.root_secondary, self.subset, self.sensor = sample_rate, root, root_secondary, subset, sensor
        self.collate_strategy, self.data_augmentation, self.batch_size = collate_strategy, data_augmentation, batch_size
        self.shuffle, self.drop_last, self.device, self.rank, self.world_size, self.seed = shuffle, drop_last, device, rank, world_size, seed
        self.max_stage_bytes = max_stage_bytes
        self.corpora: Dict[Tuple[str, str], ResidentCorpus] = {}   # (which root, split) -> resident split

    # ---- loading ---------------------------------------------------------------------------------------------------------------------
    def _load(self, root: str, subset: str, split: str, sensors) -> ResidentCorpus:
        return ResidentCorpus.load(root, subset, split, sensors, self.sample_rate, self.device, max_stage_bytes=self.max_stage_bytes)

    def setup(self, stage: Optional[str] = None) -> None:
        """Loads the splits the stage needs: ``fit`` train and validation, ``test`` test, ``None`` all three; a split already resident is
        kept."""
        splits = {"fit": ("train", "validation"), "validate": ("validation",), "test": ("test",), None: ("train", "validation", "test")}[stage]
        for split in splits:
            for which, root in (("principal", self.root), ("secondary", self.root_secondary)):
                if root is None or (which == "secondary" and split == "train") or (which, split) in self.corpora:
                    continue
                self.corpora[(which, split)] = self._load(root, self.subset, split, [AIRBORNE, self.sensor])

    def corpus(self, split: str, which: str = "principal") -> ResidentCorpus:
        if (which, split) not in self.corpora:
            raise RuntimeError(f"the {split} split of the {which} root is not loaded: call setup() with the stage that needs it first")
        return self.corpora[(which, split)]

    # ---- batches ---------------------------------------------------------------------------------------------------------------------
    def item(self, corpus: ResidentCorpus, i: int) -> Dict[str, torch.Tensor]:
        return {"audio_body_conducted": corpus.clip(i, self.sensor), "audio_airborne": corpus.clip(i, AIRBORNE)}

    def data_collator(self, batch: List[Dict[str, torch.Tensor]], deterministic: bool, collate_strategy: str) -> Dict[str, torch.Tensor]:
        return collate.bwe_collate(batch, self.sample_rate, collate_strategy, deterministic, self.data_augmentation)

    def _loader(self, corpus: ResidentCorpus, batch_size: int, deterministic: bool, train: bool) -> ResidentLoader:
        def make(indices: List[int]):
            return self.data_collator([self.item(corpus, i) for i in indices], deterministic, self.collate_strategy)
        return ResidentLoader(len(corpus), batch_size, make, shuffle=self.shuffle and train, drop_last=self.drop_last and train, seed=self.seed,
                              rank=self.rank, world_size=self.world_size)

    def _eval_loaders(self, split: str, batch_size: int):
        principal = self._loader(self.corpus(split), batch_size, True, False)
        if self.root_secondary is None:
            return principal
        return {"principal": principal, "secondary": self._loader(self.corpus(split, "secondary"), batch_size, True, False)}

    def train_dataloader(self) -> ResidentLoader:
        return self._loader(self.corpus("train"), self.batch_size, False, True)

    def val_dataloader(self):
        return self._eval_loaders("validation", min(1, self.batch_size // 4))   # bwe.py:179 (sic)

    def test_dataloader(self):
        return self._eval_loaders("test", 1)

    # ---- whole splits for EBENLightningModule.evaluate_clips -------------------------------------------------------------------------
    def _clips(self, split: str, which: str) -> Tuple[List[torch.Tensor], List[torch.Tensor]]:
        c = self.corpus(split, which)
        return c.clips(self.sensor), c.clips(AIRBORNE)

    def val_clips(self, which: str = "principal"):
        """``(corrupted, reference)`` clip lists of the validation split."""
        return self._clips("validation", which)

    def test_clips(self, which: str = "principal"):
        """``(corrupted, reference)`` clip lists of the test split: ``module.evaluate_clips(*dm.test_clips())``."""
        return self._clips("test", which)
