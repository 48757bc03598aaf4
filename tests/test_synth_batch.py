"""SceneStream.render_batch: a frame's bytes do not depend on the batch it is rendered in, so the
benchmark may render its frame pool in chunks and still feed the frames every test feeds one by one."""
import pytest
import torch

from droplet_visual_odometry_amd.synth import SceneStream

IDXS = [3, 0, 7, 8, 41]  # unordered, neighbours, far apart


def _check(w, h, device):
    st = SceneStream(w, h, device=device)
    batch = st.render_batch(IDXS)
    assert batch.shape == (len(IDXS), h, w) and batch.dtype == torch.uint8
    for j, i in enumerate(IDXS):
        assert torch.equal(batch[j], st.render(i)), i
    assert torch.equal(st.render_batch(IDXS[1:3]), batch[1:3])  # another batch size
    assert not torch.equal(batch[0], batch[1])


def test_render_batch_equals_single_frames_cpu():
    _check(320, 240, "cpu")


@pytest.mark.gpu
def test_render_batch_equals_single_frames_gpu():
    _check(640, 480, "cuda:0")
