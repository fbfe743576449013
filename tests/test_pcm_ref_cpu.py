"""CPU: the WAV header builder (data/dataset_utils.wav_header(sr, channels, subtype, n_frames)) against the standard
library's ``wave`` and scipy.io.wavfile, the RIFF pad byte, and the statistics of the dither of tests/_pcm_ref.py -- the
numpy restatement the GPU tests compare the encoder kernel with exactly."""
import io
import struct
import wave

import numpy as np
import pytest

import _pcm_ref


def _file(sr, channels, subtype, n_frames, seed=0):
    from deep_audio_mixer_amd.data import dataset_utils as du
    rng = np.random.default_rng(seed)
    payload = rng.integers(0, 256, n_frames * channels * _pcm_ref.WIDTH[subtype], dtype=np.uint8)
    if subtype == 'FLOAT':
        payload = np.ascontiguousarray(rng.standard_normal(n_frames * channels).astype('<f4')).view(np.uint8)
    head = du.wav_header(sr, channels, subtype, n_frames)
    assert head == du.build_wav_header(sr, channels, subtype, n_frames)
    return head, payload, head + payload.tobytes() + du.wav_pad(sr, channels, subtype, n_frames)


@pytest.mark.parametrize('subtype,channels,n_frames', [('PCM_16', 1, 101), ('PCM_16', 2, 1000), ('PCM_24', 2, 333),
                                                       ('PCM_24', 1, 77), ('PCM_32', 2, 64), ('PCM_32', 1, 1)])
def test_header_integer_stdlib_wave(subtype, channels, n_frames):
    head, payload, blob = _file(22050, channels, subtype, n_frames)
    assert struct.unpack('<H', head[20:22])[0] == 1                       # plain WAVE_FORMAT_PCM up to two channels
    with wave.open(io.BytesIO(blob), 'rb') as w:
        assert w.getframerate() == 22050 and w.getnchannels() == channels
        assert w.getsampwidth() == _pcm_ref.WIDTH[subtype] and w.getnframes() == n_frames
        assert w.readframes(n_frames) == payload.tobytes()


@pytest.mark.parametrize('subtype,channels', [('FLOAT', 1), ('FLOAT', 2), ('PCM_16', 6), ('PCM_24', 6), ('FLOAT', 6)])
def test_header_float_and_six_channels_scipy(subtype, channels, tmp_path):
    from scipy.io import wavfile
    from deep_audio_mixer_amd.data import dataset_utils as du
    n_frames = 257
    head, payload, blob = _file(48000, channels, subtype, n_frames)
    tag = struct.unpack('<H', head[20:22])[0]
    assert tag == (0xFFFE if channels > 2 else 3)
    if subtype == 'FLOAT':
        assert b'fact' + struct.pack('<II', 4, n_frames) in head
    path = str(tmp_path / 'x.wav')
    with open(path, 'wb') as fh:
        fh.write(blob)
    rate, data = wavfile.read(path)
    assert rate == 48000 and data.shape == ((n_frames, channels) if channels > 1 else (n_frames,))
    assert data.dtype == {'FLOAT': np.float32, 'PCM_16': np.int16, 'PCM_24': np.int32}[subtype]
    want = _pcm_ref.from_bytes(payload, subtype, channels)
    got = data.reshape(n_frames, channels)
    if subtype == 'PCM_24':
        got = got.astype(np.int64) >> 8                                  # scipy left-justifies 24-bit samples in int32
    assert np.array_equal(got.view(np.uint32) if subtype == 'FLOAT' else got,
                          want.view(np.uint32) if subtype == 'FLOAT' else want)
    # and this package's own parser (the path form of the same function)
    h = du.wav_header(path)
    assert (h['rate'], h['channels'], h['bits'], h['frames']) == (48000, channels, 8 * _pcm_ref.WIDTH[subtype], n_frames)
    assert h['tag'] == (3 if subtype == 'FLOAT' else 1) and h['data_offset'] == len(head)


def test_pad_byte_and_even_riff_size():
    from deep_audio_mixer_amd.data import dataset_utils as du
    for n_frames, padded in ((77, True), (78, False)):
        head, payload, blob = _file(44100, 1, 'PCM_24', n_frames)
        assert (len(payload) & 1) == int(padded)
        assert du.wav_pad(44100, 1, 'PCM_24', n_frames) == (b'\0' if padded else b'')
        riff_size = struct.unpack('<I', head[4:8])[0]
        assert riff_size % 2 == 0 and riff_size == len(blob) - 8
        assert struct.unpack('<I', head[-4:])[0] == len(payload)         # the data chunk's own size does not count the pad
        with wave.open(io.BytesIO(blob), 'rb') as w:
            assert w.getnframes() == n_frames
    with pytest.raises(ValueError):
        du.wav_header(44100, 2, 'PCM_8', 10)


def test_dither_statistics():
    n = 1 << 20
    zero = np.zeros((1, n), dtype=np.float32)
    streams = []
    for seed in (0, 1):
        codes, clipped = _pcm_ref.quantize(zero, 'PCM_16', dither_seed=seed)
        assert clipped.tolist() == [0]
        q = codes[:, 0]
        assert set(np.unique(q).tolist()) == {-1, 0, 1}
        for value, p in ((-1, 0.125), (0, 0.75), (1, 0.125)):
            sigma = np.sqrt(n * p * (1 - p))
            count = int((q == value).sum())
            print('seed %d: %d x %d (expected %.0f, %.2f sigma)' % (seed, count, value, n * p, (count - n * p) / sigma))
            assert abs(count - n * p) < 5 * sigma
        streams.append(q)
    assert (streams[0] != streams[1]).mean() > 0.2                       # seeds 0 and 1: different streams
    d = _pcm_ref.dither(1234, 0, 4096)
    assert np.abs(d).max() < 1.0 and abs(d.mean()) < 5 * np.sqrt(1.0 / 6.0 / 4096)       # TPDF on (-1, 1): variance 1/6


def test_dither_value_does_not_depend_on_length():
    rng = np.random.default_rng(5)
    x = (0.5 * rng.standard_normal((2, 1000))).astype(np.float32)
    long_codes, _ = _pcm_ref.quantize(x, 'PCM_24', dither_seed=99)
    short_codes, _ = _pcm_ref.quantize(x[:, :333], 'PCM_24', dither_seed=99)
    assert np.array_equal(long_codes[:333], short_codes)
    assert np.array_equal(_pcm_ref.dither(99, 100, 50), _pcm_ref.dither(99, 0, 4096)[100:150])
    plain, _ = _pcm_ref.quantize(x, 'PCM_24')
    assert np.abs(long_codes - plain).max() <= 1 and (long_codes != plain).any()


def test_quantiser_edges():
    x = np.array([[1.0, -1.0, 1.0 - 2.0 ** -15, 1.5, -1.5, np.inf, -np.inf, np.nan, 0.0, -0.0,
                   0.5 / 32768, 1.5 / 32768, 2.5 / 32768, -0.5 / 32768, -1.5 / 32768]], dtype=np.float64)
    codes, clipped = _pcm_ref.quantize(x, 'PCM_16')
    assert codes[:, 0].tolist() == [32767, -32768, 32767, 32767, -32768, 32767, -32768, 0, 0, 0, 0, 2, 2, 0, -2]
    assert clipped.tolist() == [6]                                       # 1.0, +-1.5, +-inf, NaN
    raw = _pcm_ref.to_bytes(codes, 'PCM_16')
    assert np.array_equal(_pcm_ref.from_bytes(raw, 'PCM_16', 1), codes)
    for subtype in ('PCM_24', 'PCM_32'):
        c, _ = _pcm_ref.quantize(x, subtype)
        assert np.array_equal(_pcm_ref.from_bytes(_pcm_ref.to_bytes(c, subtype), subtype, 1), c)
