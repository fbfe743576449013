"""CPU: the complex front-end and the inverse STFT are exported, and refuse every geometry outside the contract of
include/dam_hip.h BEFORE touching the device -- with null device pointers and without a GPU the answer is an error code,
never DAM_OK and never a crash."""
import pytest

OK, BAD_ARG, UNSUPPORTED = 0, -1, -2


def test_symbols_exported(dam_lib):
    for name in ('dam_stft_complex_f32', 'dam_stft_complex_strided_f32', 'dam_istft_f32', 'dam_istft_workspace_bytes'):
        assert hasattr(dam_lib, name), name


# (n_fft, hop, n_tracks, n_frames / n_samples, length)
BAD = [(2048, 0, 1, 130, 132300), (2048, 1025, 1, 130, 132300), (2048, 2048, 1, 130, 132300), (100, 25, 1, 130, 132300),
       (32768, 1024, 1, 130, 132300), (32, 8, 1, 130, 132300), (2048, 1024, -1, 130, 132300), (2048, 1024, 1, -5, 132300),
       (2048, 1024, 1, 130, -1), (2048, 1024, 0, 130, 132300), (-2048, 1024, 1, 130, 132300), (2048, -3, 1, 130, 132300)]


@pytest.mark.parametrize('n_fft,hop,n_tracks,n_frames,length', BAD)
def test_istft_validates_before_the_device(dam_lib, n_fft, hop, n_tracks, n_frames, length):
    st = dam_lib.dam_istft_f32(None, None, n_tracks, n_frames, n_fft, hop, length, None, None, None, None, 0, None)
    assert st in (BAD_ARG, UNSUPPORTED)
    assert dam_lib.dam_istft_workspace_bytes(n_tracks, n_frames, n_fft, hop, length) < 0


def test_istft_null_pointers_are_an_error(dam_lib):
    assert dam_lib.dam_istft_f32(None, None, 1, 130, 2048, 1024, 132300, None, None, None, None, 0, None) == BAD_ARG


@pytest.mark.parametrize('n_fft,hop,n_tracks,n_samples', [b[:4] for b in BAD if b[1] != 1025 and b[1] != 2048])
def test_stft_complex_validates_before_the_device(dam_lib, n_fft, hop, n_tracks, n_samples):
    # (hop > n_fft/2 is legal for the forward transform, as for torch.stft: only the inverse refuses it)
    st = dam_lib.dam_stft_complex_f32(None, 0, n_tracks, n_samples, 1, max(n_samples, 1), 1, 0, None, None, None, n_fft, hop,
                                      None, None)
    assert st in (BAD_ARG, UNSUPPORTED)


def test_stft_complex_more_refusals(dam_lib):
    f = dam_lib.dam_stft_complex_f32
    assert f(None, 0, 1, 132300, 2, 264600, 1, 0, None, None, None, 2048, 1024, None, None) == BAD_ARG       # null pointers
    assert f(None, 0, 1, 132300, 3, 396900, 1, 0, None, None, None, 2048, 1024, None, None) == UNSUPPORTED   # 3 channels
    assert f(None, 7, 1, 132300, 1, 132300, 1, 0, None, None, None, 2048, 1024, None, None) == UNSUPPORTED   # unknown dtype
    assert f(None, 0, 1, 132300, 1, 132300, 0, 0, None, None, None, 2048, 1024, None, None) == BAD_ARG       # n_sum 0
    assert f(None, 0, 1, 1024, 1, 1024, 1, 0, None, None, None, 2048, 1024, None, None) == BAD_ARG           # N <= n_fft/2
    g = dam_lib.dam_stft_complex_strided_f32
    assert g(None, 0, 59, 132300, 1, 0, 8, 2 * 7938000, 132300, 2, 1, 7938000, None, None, None, 2048, 1024, None,
             None) == BAD_ARG                                                                                  # null pointers
    assert g(None, 2, 59, 132300, 1, 0, 8, 2 * 7938000, 132300, 2, 1, 7938000, None, None, None, 2048, 1024, None,
             None) == UNSUPPORTED                                                                              # planar int16


def test_workspace_bytes_is_monotone(dam_lib):
    w = dam_lib.dam_istft_workspace_bytes
    sizes = [w(tr, 1 + n // 1024, 2048, 1024, n) for tr in (1, 8, 59, 72) for n in (16000, 132300, 220500)]
    assert all(s >= 0 for s in sizes)
    for tr in (1, 8, 59):
        for n in (16000, 132300):
            assert w(tr, 1 + n // 1024, 2048, 1024, n) <= w(tr + 13, 1 + n // 1024, 2048, 1024, n)
            assert w(tr, 1 + n // 1024, 2048, 1024, n) <= w(tr, 1 + (2 * n) // 1024, 2048, 1024, 2 * n)


def test_features_refuse_host_tensors():
    import torch
    from deep_audio_mixer_amd import features
    with pytest.raises(RuntimeError, match='GPU only'):
        features.istft(torch.zeros(1, 1025, 5, dtype=torch.complex64))
    with pytest.raises(RuntimeError, match='GPU only'):
        features.stft(torch.zeros(1, 4096))
