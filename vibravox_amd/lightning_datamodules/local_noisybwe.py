"""``NoisyBWELightningDataModule`` (vibravox/lightning_datamodules/noisybwe.py:14-291) on local recordings: every speech item of
``speech_clean`` is paired with a noise clip of ``speechless_noisy/<split>/<sensor>`` drawn as ``SpeechNoiseDataset.__getitem__`` draws
it (speech_noise.py:50, one ``torch.randint(0, n_noise, (1,))`` per item), and the batch is ``collate.noisy_bwe_collate``'s.  The draws
of a batch come in one order on the one generator: the items' noise indices in item order, then the collator's own.  The ``real``
loaders serve ``speech_noisy``: body-conducted clips only."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import torch

from .. import collate
from ..corpus import AIRBORNE
from .local_bwe import LocalBWEDataModule, ResidentLoader


class LocalNoisyBWEDataModule(LocalBWEDataModule):
    def __init__(self, sample_rate: int = 16000, root: Optional[str] = None, sensor: str = AIRBORNE, collate_strategy: str = "constant_length-2500-ms",
                 data_augmentation: Optional[torch.nn.Module] = None, batch_size: int = 32, snr_range: Optional[Sequence[float]] = None,
                 shuffle: bool = False, drop_last: bool = False, device="cuda", rank: int = 0, world_size: int = 1, seed: int = 0,
                 max_stage_bytes: int = 1 << 30, **kwargs):
        kwargs.pop("subset", None)   # the reference's config carries one; the three subsets are fixed (noisybwe.py:90-98)
        super().__init__(sample_rate=sample_rate, root=root, root_secondary=None, subset="speech_clean", sensor=sensor,
                         collate_strategy=collate_strategy, data_augmentation=data_augmentation, batch_size=batch_size, shuffle=shuffle,
                         drop_last=drop_last, device=device, rank=rank, world_size=world_size, seed=seed, max_stage_bytes=max_stage_bytes)
        self.snr_range = None if snr_range is None else tuple(snr_range)

    def setup(self, stage: Optional[str] = None) -> None:
        splits = {"fit": ("train", "validation"), "validate": ("validation",), "test": ("test",), None: ("train", "validation", "test")}[stage]
        for split in splits:
            if ("principal", split) not in self.corpora:
                self.corpora[("principal", split)] = self._load(self.root, "speech_clean", split, [AIRBORNE, self.sensor])
                self.corpora[("noise", split)] = self._load(self.root, "speechless_noisy", split, [self.sensor])
                if split != "train":
                    self.corpora[("real", split)] = self._load(self.root, "speech_noisy", split, [self.sensor])

    def data_collator(self, batch: List[Dict[str, torch.Tensor]], deterministic: bool, collate_strategy: str) -> Dict[str, torch.Tensor]:
        return collate.noisy_bwe_collate(batch, self.sample_rate, collate_strategy, deterministic, self.snr_range, self.data_augmentation)

    def _synthetic(self, split: str, batch_size: int, deterministic: bool, train: bool) -> ResidentLoader:
        speech, noise = self.corpus(split), self.corpus(split, "noise")

        def make(indices: List[int]):
            batch = []
            for i in indices:
                item = self.item(speech, i)
                item["audio_body_conducted_speechless_noisy"] = noise.clip(int(torch.randint(0, len(noise), (1,)).item()), self.sensor)
                batch.append(item)
            return self.data_collator(batch, deterministic, self.collate_strategy)
        return ResidentLoader(len(speech), batch_size, make, shuffle=self.shuffle and train, drop_last=self.drop_last and train, seed=self.seed,
                              rank=self.rank, world_size=self.world_size)

    def _real(self, split: str, batch_size: int) -> ResidentLoader:
        real = self.corpus(split, "real")

        def make(indices: List[int]):
            return self.data_collator([{"audio_body_conducted": real.clip(i, self.sensor)} for i in indices], True, self.collate_strategy)
        return ResidentLoader(len(real), batch_size, make, rank=self.rank, world_size=self.world_size)

    def train_dataloader(self) -> ResidentLoader:
        return self._synthetic("train", self.batch_size, False, True)

    def val_dataloader(self) -> Dict[str, ResidentLoader]:
        bs = min(1, self.batch_size // 4)   # noisybwe.py:172 (sic)
        return {"synthetic": self._synthetic("validation", bs, True, False), "real": self._real("validation", bs)}

    def test_dataloader(self) -> Dict[str, ResidentLoader]:
        return {"synthetic": self._synthetic("test", 1, True, False), "real": self._real("test", 1)}
