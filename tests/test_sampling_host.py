"""CPU tests of rlks.sampling's mask packers: the host packer (numpy) and the device packer (run here on CPU
tensors) write the same words, and unpack_mask inverts them."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")


def _cases(A):
    rng = np.random.default_rng(A)
    m = rng.random((5, A)) < 0.5
    m[1] = False           # a row without an allowed action
    m[2] = False
    m[2, A - 1] = True     # only the top bit (bit 63 at A = 64: the int64's sign bit)
    m[3] = True
    return m


@pytest.mark.parametrize("A", [1, 2, 63, 64])
def test_host_and_device_packers_agree_and_unpack_inverts(A):
    from rlks.sampling import pack_mask, pack_mask_device, unpack_mask

    m = _cases(A)
    host = pack_mask(m, 5, A)
    dev = pack_mask_device(torch.from_numpy(m))
    assert host.dtype == np.uint64 and dev.dtype == torch.int64 and dev.shape == (5,)
    np.testing.assert_array_equal(dev.numpy().view(np.uint64), host)
    assert int(host[1]) == 0 and int(host[2]) == 1 << (A - 1) and int(host[3]) == (1 << A) - 1
    assert [int(w) for w in host] == [sum(1 << a for a in range(A) if row[a]) for row in m]
    np.testing.assert_array_equal(unpack_mask(dev, A).numpy(), m)
    np.testing.assert_array_equal(unpack_mask(torch.from_numpy(host.view(np.int64)), A).numpy(), m)
    # a [A] row stands for n = 3 equal rows
    for row in m:
        host3 = pack_mask(row, 3, A)
        dev3 = pack_mask_device(torch.from_numpy(row).expand(3, A))
        np.testing.assert_array_equal(dev3.numpy().view(np.uint64), host3)
        assert host3.shape == (3,) and len(set(host3.tolist())) == 1
        np.testing.assert_array_equal(unpack_mask(dev3, A).numpy(), np.broadcast_to(row, (3, A)))
    # the leading shape is kept: a log's [T, N, A]
    cube = np.stack([m, ~m])
    np.testing.assert_array_equal(pack_mask_device(torch.from_numpy(cube)).numpy().view(np.uint64),
                                  np.stack([host, pack_mask(~m, 5, A)]))


def test_more_than_64_actions_is_the_same_error_from_both():
    from rlks.sampling import pack_mask, pack_mask_device

    with pytest.raises(ValueError, match="action_mask supports at most 64 actions, got 65"):
        pack_mask(np.ones((2, 65), bool), 2, 65)
    with pytest.raises(ValueError, match="action_mask supports at most 64 actions, got 65"):
        pack_mask_device(torch.ones(2, 65, dtype=torch.bool))


def test_the_moved_names_stay_importable():
    import rlks.sampling as sampling
    import rlks.serving as serving
    from rlks.ppo import PPO

    assert serving.pack_mask is sampling.pack_mask and callable(serving.check_inputs)
    assert serving.SAMPLER_ID == PPO.SAMPLER_ID == sampling.SAMPLER_ID == 0xFFFFFFFF
