"""GPU: data/dataset_utils.write_wav -- device tensors and host arrays give the same file, the file reads back (stdlib
``wave``, scipy.io.wavfile, this package's own reader) as tests/_pcm_ref.py quantises the input, a 16-bit file survives
read_wav -> write_wav byte for byte, and clipping is counted and reported."""
import wave
import warnings

import numpy as np
import pytest
import torch

import _pcm_ref

pytestmark = pytest.mark.gpu

SR, N = 22050, 12345


@pytest.fixture(scope='module')
def audio():
    rng = np.random.default_rng(8)
    return np.clip(0.3 * rng.standard_normal((2, N)), -0.99, 0.99).astype(np.float32)       # inside full scale: nothing to clip


@pytest.mark.parametrize('subtype', ['PCM_16', 'PCM_24', 'PCM_32', 'FLOAT'])
def test_read_back(dam_lib, audio, subtype, tmp_path):
    from scipy.io import wavfile
    from deep_audio_mixer_amd.data import dataset_utils as du
    p_dev, p_host = str(tmp_path / 'dev.wav'), str(tmp_path / 'host.wav')
    with warnings.catch_warnings():
        warnings.simplefilter('error')                                   # nothing clips: nothing warns
        assert du.write_wav(p_dev, torch.from_numpy(audio).cuda(), SR, subtype) == 0
        assert du.write_wav(p_host, np.ascontiguousarray(audio.T), SR, subtype) == 0
    blob = open(p_dev, 'rb').read()
    assert blob == open(p_host, 'rb').read()
    codes, _ = _pcm_ref.quantize(audio, subtype)
    want = _pcm_ref.to_bytes(codes, subtype).tobytes()
    head = du.wav_header(SR, 2, subtype, N)
    assert blob == head + want
    if subtype != 'FLOAT':
        with wave.open(p_dev, 'rb') as w:
            assert (w.getframerate(), w.getnchannels(), w.getsampwidth(), w.getnframes()) == (SR, 2, _pcm_ref.WIDTH[subtype], N)
            assert w.readframes(N) == want
    rate, data = wavfile.read(p_dev)
    assert rate == SR and data.shape == (N, 2)
    if subtype == 'FLOAT':
        assert np.array_equal(data.view(np.uint32), codes.view(np.uint32))
    else:
        assert np.array_equal(data.astype(np.int64) >> (8 if subtype == 'PCM_24' else 0), codes)
    native, rate = du.read_wav_native(p_dev)
    assert rate == SR and native.shape == (N, 2)
    if subtype == 'FLOAT':
        assert np.array_equal(native.view(np.uint32), codes.view(np.uint32))
    else:
        assert np.array_equal(native.astype(np.int64) >> (8 if subtype == 'PCM_24' else 0), codes)
    # mono: a host [frames] array and a device [n] tensor
    assert du.write_wav(p_dev, torch.from_numpy(audio[0].copy()).cuda(), SR, subtype, dither_seed=3) == 0
    assert du.write_wav(p_host, audio[0].copy(), SR, subtype, dither_seed=3) == 0
    mono = _pcm_ref.encode(audio[:1], subtype, dither_seed=3)[0].tobytes()
    assert open(p_dev, 'rb').read() == open(p_host, 'rb').read() == (
        du.wav_header(SR, 1, subtype, N) + mono + du.wav_pad(SR, 1, subtype, N))


def test_int16_round_trip(dam_lib, tmp_path):
    from scipy.io import wavfile
    from deep_audio_mixer_amd.data import dataset_utils as du
    rng = np.random.default_rng(9)
    pcm = rng.integers(-32768, 32768, (7001, 2), dtype=np.int16)
    pcm[:4, 0] = (-32768, 32767, 0, -1)
    src, dst = str(tmp_path / 'src.wav'), str(tmp_path / 'dst.wav')
    wavfile.write(src, SR, pcm)
    a, rate = du.read_wav(src, dtype=np.float32)
    assert du.write_wav(dst, a, rate, 'PCM_16') == 0
    h_src, h_dst = du.wav_header(src), du.wav_header(dst)
    raw_src = open(src, 'rb').read()[h_src['data_offset']:h_src['data_offset'] + pcm.nbytes]
    raw_dst = open(dst, 'rb').read()[h_dst['data_offset']:]
    assert raw_src == pcm.tobytes() and raw_dst == raw_src
    assert (h_dst['rate'], h_dst['channels'], h_dst['bits'], h_dst['frames']) == (SR, 2, 16, 7001)


def test_clipping_is_counted_and_warned(dam_lib, audio, tmp_path):
    from deep_audio_mixer_amd.data import dataset_utils as du
    loud = (audio * 4.0).astype(np.float32)
    loud[1, 5] = np.nan
    _, want = _pcm_ref.quantize(loud, 'PCM_16')
    assert want.sum() > 100
    path = str(tmp_path / 'loud.wav')
    with pytest.warns(RuntimeWarning, match='loud.wav') as rec:
        assert du.write_wav(path, torch.from_numpy(loud).cuda(), SR, 'PCM_16') == int(want.sum())
    assert len([w for w in rec if issubclass(w.category, RuntimeWarning)]) == 1           # once per call
    with wave.open(path, 'rb') as w:
        assert w.readframes(N) == _pcm_ref.encode(loud, 'PCM_16')[0].tobytes()
