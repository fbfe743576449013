"""GPU: mix_song_spectral (experiments.ipynb cells 44-53 for a whole song) -- ResNet18 with 4 stems in eval mode on a short
synthetic song.  The new tail (phases of the stems' sum, dam_istft_f32 with mag_db) is pinned against float64 torch on
the CPU, computed FROM THE RETURNED masked_db: max|got - want| <= 2e-6 * max|want|, the bound of tests/test_istft_gpu.py.
The head (masked against the float64 model) is what tests/test_models_gpu.py already pins; here it is compared bit for
bit with the existing public path."""
import numpy as np
import pytest
import torch

from oracle import features_ref, models_ref

pytestmark = pytest.mark.gpu

SR, N_STEMS, N_CHUNKS = 44100, 4, 7            # 7 chunks of 1 s (+ a remainder) -> 6 processed chunks of 4 x 1025 x 44
STEMS = ['s%d' % i for i in range(N_STEMS)]


def _song(seed=7, sr=SR, n_chunks=N_CHUNKS, stems=STEMS):
    rng = np.random.default_rng(seed)
    n = sr * n_chunks + 321
    t = np.arange(n) / sr
    return {s: (0.1 * rng.standard_normal((2, n)) + 0.2 * np.sin(2 * np.pi * 110.0 * (k + 1) * t)[None] *
                (0.5 + 0.5 * np.sin(2 * np.pi * 0.3 * (k + 1) * t))[None]).astype(np.float32) for k, s in enumerate(stems)}


def _dataset(tracks, stems, sr):
    from deep_audio_mixer_amd.data.dataset import MultitrackAudioDataset
    return MultitrackAudioDataset.from_arrays({'song': {**{t: tracks[t][:, :sr].T for t in stems}, 'mix': tracks[stems[0]][:, :sr].T}},
                                              tracklist=list(stems) + ['mix'], chunk_length=1, sr=sr)


def _eval_model(tracks, hop):
    """ResNet18, closed_form_fill parameters, realistic BatchNorm running statistics from two training-mode batches of real
    features on the CPU oracle, then eval mode on the GPU."""
    from deep_audio_mixer_amd.models.model_resnet import ResNet18
    torch.set_num_threads(16)
    t = 1 + SR // hop
    ref = models_ref.closed_form_fill(models_ref.RefResNet18(n_stems=N_STEMS, input_shape=(1025, t)))
    ref.train()
    with torch.no_grad():
        for c in (0, 3):
            f = np.stack([features_ref.compute_features(tracks[s][:, c * SR:(c + 1) * SR].astype(np.float64).mean(0), 2048, hop)
                          for s in STEMS])
            ref(torch.from_numpy(f[None].astype(np.float32)))
    model = ResNet18(n_stems=N_STEMS, input_shape=(1025, t))
    model.load_state_dict(ref.state_dict())
    return model.cuda().eval()


@pytest.fixture(scope='module')
def setup(dam_lib):
    from deep_audio_mixer_amd import inference_utils
    tracks = _song()
    model = _eval_model(tracks, 1024)
    yield inference_utils, model, tracks, _dataset(tracks, STEMS, SR)
    inference_utils._mixers.clear()


def _tail64(tracks, stems, masked, chunk, hop):
    """cells 50-53 in float64: phases of the STFT of the summed channel means, db_to_amplitude(masked), istft."""
    w = torch.hann_window(2048, dtype=torch.float32).double()
    out = []
    for c in range(masked.shape[0]):
        mono = sum(tracks[t][:, c * chunk:(c + 1) * chunk].astype(np.float64).mean(0) for t in stems)
        x = torch.stft(torch.from_numpy(mono), 2048, hop, window=w, center=True, return_complex=True)
        mag = x.abs()
        unit = torch.where(mag > 0, x / torch.where(mag > 0, mag, torch.ones_like(mag)), torch.ones_like(x))
        spec = torch.pow(10.0, 0.05 * torch.from_numpy(masked[c]).double()) * unit
        out.append(torch.istft(spec, 2048, hop, window=w, center=True, length=chunk).numpy())
    return np.concatenate(out)


def test_audio_matches_f64_tail(setup):
    inference_utils, model, tracks, d = setup
    audio, masked = inference_utils.mix_song_spectral(d, model, tracks, chunk_length=1, sr=SR)
    n_proc = N_CHUNKS - 1
    assert audio.shape == (n_proc * SR,) and audio.dtype == np.float32
    assert masked.shape == (n_proc, 1025, 44) and masked.dtype == np.float32
    assert np.isfinite(masked).all() and np.isfinite(audio).all()
    want = _tail64(tracks, STEMS, masked, SR, 1024)
    err, peak = np.abs(audio.astype(np.float64) - want).max(), np.abs(want).max()
    print('spectral tail: masked in [%.1f, %.1f] dB, max err %.3e of peak %.3e = %.3e' % (masked.min(), masked.max(), err, peak, err / peak))
    assert peak > 0 and err <= 2e-6 * peak
    assert np.std(masked.mean(axis=(1, 2))) > 0          # the chunks differ
    a64, _ = inference_utils.mix_song_spectral(d, model, tracks, chunk_length=1, sr=SR, dtype=np.float64)
    assert a64.dtype == np.float64 and np.array_equal(a64, audio.astype(np.float64))


def test_audio_matches_f64_tail_hop_512(dam_lib):
    """The same independent end-to-end check at the hop of the notebook's cell 53 (hop_length=512): eval-mode model of its
    own geometry (1025 x 87), float64 phases computed on the CPU from the song, bound as above."""
    from deep_audio_mixer_amd import inference_utils
    tracks = _song(seed=9)
    model = _eval_model(tracks, 512)
    audio, masked = inference_utils.mix_song_spectral(_dataset(tracks, STEMS, SR), model, tracks, chunk_length=1, sr=SR,
                                                      hop_length=512)
    assert masked.shape == (N_CHUNKS - 1, 1025, 87) and audio.shape == ((N_CHUNKS - 1) * SR,)
    assert next(iter(inference_utils._mixers.values())).graph is not None
    want = _tail64(tracks, STEMS, masked, SR, 512)
    err, peak = np.abs(audio.astype(np.float64) - want).max(), np.abs(want).max()
    print('spectral tail hop 512: masked in [%.1f, %.1f] dB, max err %.3e of peak %.3e = %.3e' % (masked.min(), masked.max(), err, peak, err / peak))
    assert peak > 0 and err <= 2e-6 * peak
    inference_utils._mixers.clear()


def test_masked_is_the_public_forward_and_graph_equals_eager(setup):
    inference_utils, model, tracks, d = setup
    from deep_audio_mixer_amd import features
    audio, masked = inference_utils.mix_song_spectral(d, model, tracks, chunk_length=1, sr=SR)
    mixer = next(iter(inference_utils._mixers.values()))
    assert mixer.kind == 'spectral' and mixer.graph is not None and mixer.n_proc == N_CHUNKS - 1
    graph = mixer.graph
    pcm = torch.from_numpy(np.stack([tracks[t] for t in STEMS])).cuda()
    with torch.no_grad():
        feats = features.stft_logmag_song_chunks(pcm, N_CHUNKS - 1, SR)
        want = model(feats.view(N_CHUNKS - 1, N_STEMS, 1025, 44))[0].cpu().numpy()
    assert np.array_equal(masked, want)
    audio2, masked2 = inference_utils.mix_song_spectral(d, model, tracks, chunk_length=1, sr=SR)       # replay
    assert next(iter(inference_utils._mixers.values())).graph is graph
    assert np.array_equal(audio2, audio) and np.array_equal(masked2, masked)
    eager = inference_utils.SongMixer(model, N_STEMS, 2, pcm.shape[2], torch.float32, SR, 'spectral', use_graph=False)
    audio3, masked3 = eager.run([tracks[t] for t in STEMS])
    assert eager.graph is None
    assert np.array_equal(audio3, audio) and np.array_equal(masked3, masked)
    # another song through the same graph
    tracks_b = {t: np.ascontiguousarray(v[:, ::-1]) for t, v in tracks.items()}
    audio_b, _ = inference_utils.mix_song_spectral(d, model, tracks_b, chunk_length=1, sr=SR)
    assert next(iter(inference_utils._mixers.values())).graph is graph
    assert np.array_equal(audio_b, eager.run([tracks_b[t] for t in STEMS])[0]) and not np.array_equal(audio_b, audio)


def test_parameter_update_is_picked_up(setup):
    """The captured forward holds folded conv + BatchNorm images: parameters changed in place between two calls of the same
    geometry must lead to the new result, not a replay of the old weights."""
    inference_utils, model, tracks, d = setup
    audio, masked = inference_utils.mix_song_spectral(d, model, tracks, chunk_length=1, sr=SR)
    state = {k: v.clone() for k, v in model.state_dict().items()}
    try:
        with torch.no_grad():
            for p in model._heads.parameters():
                p.mul_(1.05)
            model.layer6[1].conv2.weight.mul_(1.05)
        audio_u, masked_u = inference_utils.mix_song_spectral(d, model, tracks, chunk_length=1, sr=SR)
        n = tracks[STEMS[0]].shape[1]
        fresh = inference_utils.SongMixer(model, N_STEMS, 2, n, torch.float32, SR, 'spectral', use_graph=False)
        audio_f, masked_f = fresh.run([tracks[t] for t in STEMS])
        assert np.array_equal(masked_u, masked_f) and np.array_equal(audio_u, audio_f)
        assert not np.array_equal(masked_u, masked)
    finally:
        with torch.no_grad():
            model.load_state_dict(state)


def test_training_mode_two_chunks_and_hop_512(dam_lib):
    """A model left in training mode runs chunk by chunk, eagerly (batch statistics per call, as the reference's loop); a
    song of two chunks is valid here (nothing is smoothed); hop_length reaches the front-end."""
    from deep_audio_mixer_amd import features, inference_utils
    from deep_audio_mixer_amd.models.model_resnet import ResNet18
    sr, hop, stems = 16000, 512, ['bass', 'drums']
    t = 1 + sr // hop
    torch.manual_seed(2)
    model = ResNet18(n_stems=2, input_shape=(1025, t)).cuda().train()
    for n_chunks in (2, 5):
        tracks = _song(seed=n_chunks, sr=sr, n_chunks=n_chunks, stems=stems)
        d = _dataset(tracks, stems, sr)
        before = model.bn1.num_batches_tracked.item()
        audio, masked = inference_utils.mix_song_spectral(d, model, tracks, chunk_length=1, sr=sr, hop_length=hop)
        n_proc = n_chunks - 1
        assert model.bn1.num_batches_tracked.item() == before + n_proc
        assert next(iter(inference_utils._mixers.values())).graph is None
        assert audio.shape == (n_proc * sr,) and masked.shape == (n_proc, 1025, t)
        pcm = torch.from_numpy(np.stack([tracks[s] for s in stems])).cuda()
        with torch.no_grad():
            feats = features.stft_logmag_song_chunks(pcm, n_proc, sr, 2048, hop).view(n_proc, 2, 1025, t)
            for c in range(n_proc):
                assert np.array_equal(model(feats[c:c + 1])[0][0].cpu().numpy(), masked[c])
        # The tail in its two steps, each at its own bound.  (An untrained model's `masked` is not shaped like the input
        # spectrum: it gives bins whose |X| is far below the frame peak full weight, and the phase of such a bin is only as
        # good as the forward error relative to |X|, not to the peak -- so here the float64 tail is rebuilt from the
        # phase source the device used, and that phase source is checked against float64 as the forward transform is.)
        spec = next(iter(inference_utils._mixers.values())).spec.cpu()
        w = torch.hann_window(2048, dtype=torch.float32).double()
        for c in range(n_proc):
            mono = sum(tracks[s][:, c * sr:(c + 1) * sr].astype(np.float64).mean(0) for s in stems)
            x = torch.stft(torch.from_numpy(mono), 2048, hop, window=w, center=True, return_complex=True)
            assert ((spec[c].to(torch.complex128) - x).abs() / x.abs().amax(0, keepdim=True)).max().item() <= 2e-6
            xs = spec[c].to(torch.complex128)
            mag = xs.abs()
            unit = torch.where(mag > 0, xs / torch.where(mag > 0, mag, torch.ones_like(mag)), torch.ones_like(xs))
            want = torch.istft(torch.pow(10.0, 0.05 * torch.from_numpy(masked[c]).double()) * unit, 2048, hop, window=w,
                               center=True, length=sr).numpy()
            assert np.abs(audio[c * sr:(c + 1) * sr] - want).max() <= 2e-6 * np.abs(want).max()
    with pytest.raises(ValueError):             # the gain kinds keep their Savitzky-Golay window check
        inference_utils.mix_song_smooth(d, model, _song(seed=1, sr=sr, n_chunks=2, stems=stems), chunk_length=1, sr=sr)
    inference_utils._mixers.clear()
