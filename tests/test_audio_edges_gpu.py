"""avt_spectrogram (avt_amd.audio.spectrogram) at its edges against scipy.signal.spectrogram in
float64 (oracle/audio_oracle.py): segment counts around the SG_SPB = 8 segments a block handles,
hops other than the reference's 511, B = 1 and 1-D input, odd clip lengths, extreme signals, the
1 / fs density scaling, and the independence of the clips of a batch.  The bound is the project's
(tests/test_audio_gpu.py): max |d| < 5e-5 in normalised-log units."""
import numpy as np
import pytest
import torch

import audio_oracle as ao
from avt_amd.audio import num_segments, spectrogram

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
TOL = 5e-5
FLOOR = float(np.log(1e-7) / 12.0)


def _run(waves, sr, **kw):
    return spectrogram(torch.from_numpy(waves).to(DEV), sr, **kw).cpu().numpy()


def _compare(got, waves, sr, noverlap=1, tag=""):
    """got [B, 1, 257, nseg] against scipy on each (clipped, float64) row of waves [B, N]."""
    waves = np.atleast_2d(waves)
    assert got.shape[:3] == (waves.shape[0], 1, 257) and got.dtype == np.float32
    for b in range(waves.shape[0]):
        ref = ao.reference_spectrogram(np.clip(waves[b].astype(np.float64), -1, 1), sr, noverlap)
        assert got[b].shape == ref.shape, (tag, b, got[b].shape, ref.shape)
        err = np.abs(got[b] - ref).max()
        print(f"{tag} row {b}: max |d| = {err:.2e} (normalised log units)")
        assert err < TOL, (tag, b, err)


def _mix(B, n, sr, seed):
    """Rows of noise, a clipping row and a tone, as in test_audio_gpu."""
    rng = np.random.default_rng(seed)
    w = 0.3 * rng.standard_normal((B, n))
    w[0] *= 5.0
    if B > 1:
        w[1] = 0.5 * np.sin(2 * np.pi * 440.0 * np.arange(n) / sr) + 1e-3 * rng.standard_normal(n)
    return w.astype(np.float32)


@pytest.mark.parametrize("form", ["1d", "B1", "B3"])
@pytest.mark.parametrize("n,nseg", [(512, 1), (512 + 511 * 7, 8), (512 + 511 * 8, 9), (512 + 511 * 8 + 510, 9),
                                    (512 + 511 * 15, 16)])
def test_segment_counts_around_a_block(n, nseg, form):
    """nseg = 1, 8 (one full block), 9 (a block of one), 9 with 510 unused samples, 16 (two full)."""
    sr = 16000
    waves = _mix(3 if form == "B3" else 1, n, sr, 100 + n)
    scipy_cols = ao.reference_spectrogram(waves[0].astype(np.float64), sr).shape[2]
    assert num_segments(n) == scipy_cols == nseg
    got = _run(waves[0] if form == "1d" else waves, sr)
    assert got.shape == (waves.shape[0], 1, 257, nseg)
    _compare(got, waves, sr, tag=f"n={n} {form}")


def test_too_short_is_refused():
    assert num_segments(511) == 0
    for shape in [(511,), (1, 511), (3, 511)]:
        with pytest.raises(ValueError, match="at least 512"):
            spectrogram(torch.zeros(shape, device=DEV), 16000)


@pytest.mark.parametrize("noverlap,n", [(0, 512 * 9 + 100), (256, 512 + 256 * 8 + 37), (511, 512 + 40)])
def test_other_hops(noverlap, n):
    """Hops 512, 256 and 1 (the wrapper's noverlap), nseg = 9, 9 and 41."""
    sr = 16000
    waves = _mix(2, n, sr, 200 + noverlap)
    hop = 512 - noverlap
    assert num_segments(n, noverlap=noverlap) == (n - 512) // hop + 1
    got = _run(waves, sr, noverlap=noverlap)
    assert got.shape[3] == num_segments(n, noverlap=noverlap)
    _compare(got, waves, sr, noverlap, tag=f"noverlap={noverlap}")


def _signals(n, sr):
    t = np.arange(n)
    square = np.where((t % 8) < 4, 1.0, -1.0)   # full scale, fundamental at sr / 8: the largest power
    impulse = np.zeros(n)
    impulse[255] = 1.0
    return np.stack([square, np.full(n, 0.7), np.full(n, 3.0), impulse]).astype(np.float32)


def test_extreme_signals_in_one_launch():
    """B = 4, N odd: a full-scale square wave (the 1e-7 floor is irrelevant at its peaks), constants
    0.7 and 3.0 (3.0 clips to 1; both detrend to exactly 0, so every bin is log(1e-7) / 12) and a
    single impulse (a flat spectrum a little above the floor)."""
    n, sr = 512 + 511 * 8 + 1, 16000
    waves = _signals(n, sr)
    got = _run(waves, sr)
    assert got.shape == (4, 1, 257, 9)
    _compare(got, waves, sr, tag="signals")
    assert got[0].max() > FLOOR + 0.5  # the square wave's lines stand far above the floor
    for b in (1, 2):
        assert np.abs(got[b] - FLOOR).max() < 1e-6, b
    assert np.abs(got[3][..., 1:] - FLOOR).max() < 1e-6  # the impulse is in segment 0 only
    assert got[3][..., 0].min() > FLOOR + 1e-3


@pytest.mark.parametrize("sr", [1.0, 16000, 48000])
def test_noise_near_the_floor_and_density_scaling(sr):
    """White noise of amplitude 1e-4: PSD ~ 2e-8 / fs, next to the 1e-7 floor at fs = 1 and far
    below it at 16 and 48 kHz (the scaling is 1 / fs)."""
    n = 512 + 511 * 9 + 3
    waves = (1e-4 * np.random.default_rng(300).standard_normal((4, n))).astype(np.float32)
    got = _run(waves, sr)
    _compare(got, waves, sr, tag=f"noise sr={sr}")
    if sr == 1.0:
        assert got.max() > FLOOR + 1e-3  # the noise is visible here, so the 1 / fs factor is tested


@pytest.mark.parametrize("n", [1533, 512 + 511 * 8 + 1])
def test_clips_of_a_batch_are_independent(n):
    """Row b of a B = 3 launch equals, bit for bit, that row run alone; N odd, so rows 1 and 2 start
    at odd float offsets."""
    sr = 16000
    waves = _mix(3, n, sr, 400 + n)
    both = spectrogram(torch.from_numpy(waves).to(DEV), sr)
    for b in range(3):
        alone = spectrogram(torch.from_numpy(waves[b:b + 1].copy()).to(DEV), sr)
        assert torch.equal(both[b:b + 1], alone), b
    _compare(both.cpu().numpy(), waves, sr, tag=f"batch n={n}")
