"""The frequency encoder's host side: the factory, the C ABI's argument checks (no launch), main_nerf's flag and the networks that
take 'frequency' for their encoders.  No GPU."""
import os
import re

import pytest
import torch

from nerfsafetyvalidation_amd import _lib, main_nerf
from nerfsafetyvalidation_amd.encoding import get_encoder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000          # a non-null "device pointer": the calls below are refused before anything reads it


def test_factory_returns_the_frequency_encoder():
    from nerfsafetyvalidation_amd.freqencoder import FreqEncoder
    enc, dim = get_encoder("frequency", input_dim=3, multires=6)
    assert isinstance(enc, FreqEncoder) and dim == 39 and enc.output_dim == 39 and enc.degree == 6 and enc.input_dim == 3
    assert get_encoder("frequency", input_dim=2, multires=6)[1] == 26
    assert get_encoder("frequency")[1] == 39                                        # the reference's defaults: input_dim 3, multires 6
    for input_dim in (1, 2, 3, 5):
        assert FreqEncoder(input_dim=input_dim, degree=0).output_dim == input_dim
        assert get_encoder("frequency", input_dim=input_dim, multires=0)[1] == input_dim
    assert FreqEncoder().output_dim == 27                                           # freq.py:56: degree 4
    assert repr(FreqEncoder(input_dim=2, degree=3)) == "FreqEncoder: input_dim=2 degree=3 output_dim=14"
    assert list(enc.parameters()) == []
    with pytest.raises(NotImplementedError, match="frequency"):                     # the list of choices names it
        get_encoder("ash")
    with pytest.raises(AssertionError):
        FreqEncoder(degree=17)


def test_cpu_tensors_are_refused():
    from nerfsafetyvalidation_amd.freqencoder import FreqEncoder, freq_encode
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        FreqEncoder(3, 4)(torch.zeros(5, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        freq_encode(torch.zeros(5, 3), 4, 27)
    with pytest.raises(ValueError, match="output_dim"):
        freq_encode(torch.zeros(5, 3), 4, 24)


def test_header_and_bindings_agree():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ngp_hip.h")).read(), flags=re.S)
    fwd = re.search(r"NGP_API int ngp_freq_encode_forward\((.*?)\);", text, flags=re.S).group(1)
    bwd = re.search(r"NGP_API int ngp_freq_encode_backward\((.*?)\);", text, flags=re.S).group(1)
    assert [a.split()[-1] for a in fwd.split(",")] == ["inputs", "outputs", "B", "D", "deg", "stream"]
    assert [a.split()[-1] for a in bwd.split(",")] == ["grad", "inputs", "B", "D", "deg", "grad_inputs", "stream"]
    assert len(_lib.SIGNATURES["ngp_freq_encode_forward"]) == 6 and len(_lib.SIGNATURES["ngp_freq_encode_backward"]) == 7
    lib = _lib.lib()
    assert lib.ngp_freq_encode_forward.restype is _lib.C.c_int and lib.ngp_freq_encode_backward.restype is _lib.C.c_int


def test_argument_checks_launch_nothing():
    lib = _lib.lib()
    assert lib.ngp_freq_encode_forward(FAKE, FAKE, 8, 3, 17, None) == -1                                 # NGP_EINVAL
    assert b"freq_encode_forward" in lib.ngp_last_error() and b"degree 17" in lib.ngp_last_error()
    assert lib.ngp_freq_encode_forward(None, FAKE, 8, 3, 4, None) == -1
    assert lib.ngp_last_error() == b"freq_encode_forward: null pointer"
    assert lib.ngp_freq_encode_forward(FAKE, None, 8, 3, 4, None) == -1
    assert lib.ngp_last_error() == b"freq_encode_forward: null pointer"
    assert lib.ngp_freq_encode_forward(FAKE, FAKE, 8, 0, 4, None) == -1 and b"input dim" in lib.ngp_last_error()
    assert lib.ngp_freq_encode_backward(FAKE, FAKE, 8, 3, 17, FAKE, None) == -1
    assert b"freq_encode_backward" in lib.ngp_last_error() and b"degree 17" in lib.ngp_last_error()
    for args in ((None, FAKE, 8, 3, 4, FAKE), (FAKE, None, 8, 3, 4, FAKE), (FAKE, FAKE, 8, 3, 4, None)):
        assert lib.ngp_freq_encode_backward(*args, None) == -1
        assert lib.ngp_last_error() == b"freq_encode_backward: null pointer"
    # no rows: success without a launch, whatever the pointers
    assert lib.ngp_freq_encode_forward(None, None, 0, 3, 4, None) == 0
    assert lib.ngp_freq_encode_backward(None, None, 0, 3, 16, None, None) == 0


def test_parser_knows_encoding_dir():
    assert main_nerf.parse_args(["data"]).encoding_dir == "sphere_harmonics"
    assert main_nerf.parse_args(["data", "--encoding_dir", "frequency"]).encoding_dir == "frequency"
    assert main_nerf.parse_args(["data", "--ff"]).encoding_dir == "sphere_harmonics"
    with pytest.raises(AssertionError, match="encoding_dir"):
        main_nerf.parse_args(["data", "--encoding_dir", "frequency", "--ff"])
    with pytest.raises(SystemExit):
        main_nerf.parse_args(["data", "--encoding_dir", "ash"])


def test_networks_take_the_frequency_encoders():
    from nerfsafetyvalidation_amd.freqencoder import FreqEncoder
    from nerfsafetyvalidation_amd.nerf.network import NeRFNetwork
    net = NeRFNetwork(encoding_dir="frequency")
    assert isinstance(net.encoder_dir, FreqEncoder) and net.in_dim_dir == 39
    assert net.color_net[0].in_features == 39 + 15 and net.sigma_net[0].in_features == 32
    assert net.fused_model() is None
    net = NeRFNetwork(encoding="frequency")
    assert isinstance(net.encoder, FreqEncoder) and net.sigma_net[0].in_features == 39 and net.color_net[0].in_features == 16 + 15
    assert net.fused_model() is None
    net = NeRFNetwork(bg_radius=1, encoding_bg="frequency")
    assert isinstance(net.encoder_bg, FreqEncoder) and net.encoder_bg.input_dim == 2 and net.bg_net[0].in_features == 26 + 16
    assert net.fused_model() is None
    # the state-keeping entry points with an encoder that has no table
    net = NeRFNetwork(encoding="frequency", encoding_dir="frequency")
    net.invalidate_fused()
    net.train()
    net.eval()
    other = NeRFNetwork(encoding="frequency", encoding_dir="frequency")
    res = other.load_state_dict(net.state_dict())
    assert not res.missing_keys and not res.unexpected_keys
    assert torch.equal(other.color_net[0].weight, net.color_net[0].weight)
    assert [len(list(g["params"])) for g in net.get_params(1e-2)] == [0, 2, 0, 3]
    assert net.fused_model() is None


def test_the_fully_fused_network_refuses_it():
    from nerfsafetyvalidation_amd.nerf.network_ff import NeRFNetwork
    with pytest.raises(NotImplementedError, match="frequency"):
        NeRFNetwork(encoding_dir="frequency")
