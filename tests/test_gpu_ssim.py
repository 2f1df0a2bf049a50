"""so_ssim_u8 on the GPU against tests/ssimref.py (absolute 1e-9, the project's PSNR tolerance):
shapes around the 16 x 64 tile of window positions, every content kind, windows 11 / 7 / 3,
pitched views, bit-exact determinism, and the opt-in ssim=True paths of the codec."""
import numpy as np
import pytest
import torch

import ssimref

pytestmark = pytest.mark.gpu

TH, TW = 16, 64   # so_ssim.hip: window positions per tile
TOL = 1e-9
# one window; small; wide and flat; exactly one tile; one row and one column more; several
# tiles with cut edges; more tiles (32 x 17 = 544) than the final reduction has threads (256)
SHAPES = [(11, 11), (16, 16), (12, 75), (TH + 10, TW + 10), (TH + 11, TW + 11), (70, 130), (520, 1040)]


@pytest.fixture(scope="module")
def eng(gpu):
    from streamoptima_amd.engine import Engine
    return Engine(64, 128, 16, 16, False, 0.015, gpu)


def _dev(x, gpu):
    return torch.from_numpy(np.ascontiguousarray(x)).to(gpu)


@pytest.mark.parametrize("h,w", SHAPES)
def test_kernel_matches_ssimref_win11(gpu, eng, h, w):
    pairs = [ssimref.contents(kind, h, w, seed=7 * h + w + k) for k, kind in enumerate(ssimref.KINDS)]
    got = eng.ssim([_dev(a, gpu) for a, _ in pairs], [_dev(b, gpu) for _, b in pairs], h, w).cpu().numpy()
    for kind, (a, b), g in zip(ssimref.KINDS, pairs, got):
        want = ssimref.ssimref(a, b)
        print(f"{h}x{w} {kind}: got {g!r} want {want!r} diff {abs(g - want):.3e}")
        assert abs(g - want) <= TOL, (kind, g, want)
    assert got[ssimref.KINDS.index("same")] == 1.0                      # exactly
    assert abs(got[ssimref.KINDS.index("extreme")] - ssimref.C1 / (65025 + ssimref.C1)) <= TOL


@pytest.mark.parametrize("win", [7, 3])
@pytest.mark.parametrize("h,w", [(12, 75), (70, 130)])
def test_kernel_other_windows(gpu, eng, h, w, win):
    pairs = [ssimref.contents(kind, h, w, seed=11 * h + w + win + k) for k, kind in enumerate(ssimref.KINDS)]
    got = eng.ssim([_dev(a, gpu) for a, _ in pairs], [_dev(b, gpu) for _, b in pairs], h, w, win=win).cpu().numpy()
    for kind, (a, b), g in zip(ssimref.KINDS, pairs, got):
        want = ssimref.ssimref(a, b, win)
        print(f"{h}x{w} win {win} {kind}: got {g!r} want {want!r} diff {abs(g - want):.3e}")
        assert abs(g - want) <= TOL, (kind, win, g, want)
    assert got[ssimref.KINDS.index("same")] == 1.0


def test_pitched_views(gpu, eng):
    """h x w views at odd offsets inside larger buffers whose surroundings differ between a and b:
    only the views may count."""
    h, w = 45, 83
    for k, (oy, ox, bh, bw) in enumerate([(3, 5, 60, 101), (0, 1, 45, 90), (7, 2, 64, 85)]):
        a, b = ssimref.contents("near", h, w, seed=40 + k)
        big_a = torch.full((bh, bw), 17, dtype=torch.uint8, device=gpu)
        big_b = torch.full((bh, bw + 3), 201, dtype=torch.uint8, device=gpu)   # another pitch on the b side
        va, vb = big_a[oy:oy + h, ox:ox + w], big_b[oy + 0:oy + h, ox + 1:ox + 1 + w]
        va.copy_(_dev(a, gpu))
        vb.copy_(_dev(b, gpu))
        got = float(eng.ssim([va], [vb], h, w).cpu()[0])
        want = ssimref.ssimref(a, b)
        print(f"view {k}: got {got!r} want {want!r} diff {abs(got - want):.3e}")
        assert abs(got - want) <= TOL
        # and the picture area of a larger plane, as encode_device measures padded frames
        got = float(eng.ssim([big_a], [big_b[:, :bw]], oy + h, ox + w).cpu()[0])
        want = ssimref.ssimref(big_a.cpu().numpy()[:oy + h, :ox + w], big_b.cpu().numpy()[:oy + h, :ox + w])
        assert abs(got - want) <= TOL


def test_deterministic_and_batch_independent(gpu):
    """NaN in the workspace before every call; a batch of 3 frames twice, and each frame alone:
    the same bits."""
    from streamoptima_amd import _lib
    from streamoptima_amd.engine import ssim_planes
    lib = _lib.load()
    h, w = 70, 300
    pairs = [ssimref.contents(kind, h, w, seed=60 + k) for k, kind in enumerate(("noise", "near", "wrap"))]
    a, b = [_dev(x, gpu) for x, _ in pairs], [_dev(y, gpu) for _, y in pairs]
    need = lib.so_ssim_workspace_elems(3, h, w, 11)
    assert need == 3 * lib.so_ssim_workspace_elems(1, h, w, 11) > 3
    ws = torch.empty(need, dtype=torch.float64, device=gpu)

    def run(ia):
        ws.fill_(float("nan"))
        return ssim_planes(lib, gpu, [a[i] for i in ia], [b[i] for i in ia], h, w, 11, None, ws).cpu().numpy()
    first, second = run([0, 1, 2]), run([0, 1, 2])
    assert np.isfinite(first).all()
    assert first.tobytes() == second.tobytes()
    for i in range(3):
        assert run([i]).tobytes() == first[i:i + 1].tobytes(), i
        assert abs(first[i] - ssimref.ssimref(*pairs[i])) <= TOL
    assert run([2, 0]).tobytes() == first[[2, 0]].tobytes()


def _codec(gpu, h, w, seq, ssim):
    from streamoptima_amd.Encoder import Y_Video_codec
    c = Y_Video_codec(h, w, len(seq), 16, 16, 4, 4, 0, 0.015, False, y_only_frame_arr=seq, device=gpu, ssim=ssim)
    c.recon_yuv_path = "/nonexistent-dir/x.yuv"   # no file output
    return c


def test_small_gop_through_encode(gpu):
    """64 x 128, 5 frames, intra_dur 4 (W % 128 == 0: the persistent P-run): the package's SSIM
    is ssimref(frame, recon), and nothing else moves against an ssim=False encode."""
    from streamoptima_amd.synth import synth_sequence
    seq = synth_sequence(5, 64, 128, seed=5)
    on, off = _codec(gpu, 64, 128, seq, True), _codec(gpu, 64, 128, seq, False)
    psnr_on, psnr_off = on.encode(), off.encode()
    assert psnr_on == psnr_off
    ssim = on.encoded_package["SSIM per frame"]
    assert ssim == on.ssim_per_frame and len(ssim) == 5 and all(isinstance(v, float) for v in ssim)
    assert all(np.isnan(v) for v in off.encoded_package["SSIM per frame"]) and off.ssim_per_frame is None
    for i, (s_on, s_off) in enumerate(zip(on._symbols, off._symbols)):
        recon = s_on.recon.cpu().numpy()
        assert np.array_equal(recon, s_off.recon.cpu().numpy()), i
        want = ssimref.ssimref(seq[i], recon)
        print(f"frame {i}: got {ssim[i]!r} want {want!r} diff {abs(ssim[i] - want):.3e}")
        assert abs(ssim[i] - want) <= TOL, i
    res_on = on.encode_device(on._upload_padded(seq), 4)
    assert "ssim" in res_on and res_on["ssim"].dtype == torch.float64 and res_on["ssim"].shape == (5,)
    assert res_on["ssim"].cpu().tolist() == ssim
    assert "ssim" not in off.encode_device(off._upload_padded(seq), 4)
    g_on = on.encode_gops_device([on._upload_padded(seq)], 4)[0]
    assert g_on["ssim"].cpu().tolist() == ssim
    assert "ssim" not in off.encode_gops_device([off._upload_padded(seq)], 4)[0]


def test_padded_gop(gpu):
    """60 x 100 padded to 64 x 112: the SSIM is over the picture, not the padding."""
    from streamoptima_amd.synth import synth_sequence
    seq = synth_sequence(3, 64, 112, seed=9)[:, :60, :100]
    c = _codec(gpu, 60, 100, np.ascontiguousarray(seq), True)
    c.encode()
    for i, s in enumerate(c._symbols):
        recon = s.recon.cpu().numpy()
        assert recon.shape == (64, 112)
        want = ssimref.ssimref(seq[i], recon[:60, :100])
        got = c.encoded_package["SSIM per frame"][i]
        print(f"frame {i}: got {got!r} want {want!r} diff {abs(got - want):.3e}")
        assert abs(got - want) <= TOL, i


def test_calculate_metrics_with_ssim(gpu):
    a, b = ssimref.contents("near", 288, 352, seed=77)
    seq = np.zeros((1, 64, 128), np.uint8)
    c = _codec(gpu, 64, 128, seq, True)
    psnr, ssim = c.calculate_metrics(a, b.astype(np.float64))
    mse = float(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))
    assert psnr == pytest.approx(10 * np.log10(255 ** 2 / mse), abs=1e-9)
    assert abs(ssim - ssimref.ssimref(a, b)) <= TOL
    with pytest.raises(ValueError):
        c.calculate_metrics(a[:10], b[:10])
    with pytest.raises(ValueError):
        c.calculate_metrics(a[:, :10], b[:, :10])
    psnr_off, ssim_off = _codec(gpu, 64, 128, seq, False).calculate_metrics(a, b)
    assert psnr_off == psnr and np.isnan(ssim_off)
