"""CPU: batch-normalised layers (batch_normalize: true) — the host builds them with the reference's configuration, refuses what it
does not support with a reason, exports the entry points, and tests/bn_ref.py (the float64 restatement the GPU tests compare
against) is the true batch-norm gradient where the reference's sequence is one."""
import numpy as np
import pytest

from convnet_amd import _lib, models
from convnet_amd.convnet import ConvNet
from convnet_amd.grad_check import GradChecker

import bn_ref

BN_LAYERS = ("conv1", "conv2", "fc3")


def test_small_bn_net_builds_with_the_reference_configuration():
    net = ConvNet(models.small_bn(bn_f=0.9))
    by = {l.GetName(): l for l in net.layers_}
    for name in BN_LAYERS:
        l = by[name]
        assert l.UseBatchNormalization()
        assert np.float32(l.bn_f_) == np.float32(0.9) and np.float32(l.bn_epsilon_) == np.float32(1e-5)   # proto default eps
        assert l.gamma_optimizer_ is not None and l.beta_optimizer_ is not None
        assert l.gamma_optimizer_.epsilon_ == 0.01 and l.beta_optimizer_.epsilon_ == 0.01
    assert not any(by[n].UseBatchNormalization() for n in ("input", "pool1", "output"))
    assert net.GetLayerByName("conv2").dropprob_ > 0


def test_vgg_bn_normalises_every_conv_layer():
    net = ConvNet(models.vgg_bn())
    bn = [l.GetName() for l in net.layers_ if l.UseBatchNormalization()]
    assert bn == [l.GetName() for l in net.layers_ if l.GetName().startswith("conv")] and len(bn) == 13
    plain = ConvNet(models.vgg())
    assert [l.GetName() for l in plain.layers_] == [l.GetName() for l in net.layers_]


def test_bn_entries_are_exported():
    names = set(_lib.declared_symbols())
    for n in ("bn_bprop_inplace", "bn_bprop", "bn_grad", "bn_fprop_act", "bn_bprop_fused"):
        assert n in names and hasattr(_lib.lib, n), n


def test_beta_optimizer_block_is_ignored_like_the_reference():
    # src/convnet.cc:56-64 merges the layer's beta_optimizer into the gamma config's copy: beta runs the default bias optimizer
    text = models.small_bn().replace("  batch_normalize: true\n",
                                     "  batch_normalize: true\n  gamma_optimizer { epsilon: 0.3 }\n  beta_optimizer { epsilon: 0.7 }\n", 1)
    text = text.replace("default_bias_optimizer {\n  epsilon: 0.01", "default_bias_optimizer {\n  epsilon: 0.02", 1)
    net = ConvNet(text)
    l = net.GetLayerByName("conv1")
    assert l.gamma_optimizer_.epsilon_ == 0.3
    assert l.gamma_optimizer_.final_momentum_ == 0.9   # the rest of gamma's config: the default weight optimizer
    assert l.beta_optimizer_.epsilon_ == 0.02


def _bn(text, layer):
    return text.replace(f'  name: "{layer}"\n', f'  name: "{layer}"\n  batch_normalize: true\n', 1)


@pytest.mark.parametrize("text, why", [
    (_bn(models.small_bn(), "input"), "input and output"),
    (_bn(models.small_bn(), "output"), "input and output"),
    (_bn(models.alexnet(), "hidden1_maxpool"), "MaxPoolEdge"),
    (_bn(models.alexnet(), "hidden1_rnorm"), "ResponseNormEdge"),
], ids=["input", "output", "maxpool-fed", "rnorm-fed"])
def test_unsupported_batch_norm_layers_are_refused(text, why):
    with pytest.raises(SystemExit, match=why):
        ConvNet(text)


def test_batch_norm_is_refused_with_a_gradient_exchange_and_in_the_grad_checker():
    with pytest.raises(SystemExit, match="gradient exchange"):
        ConvNet(models.small_bn(), exchange=object())
    with pytest.raises(SystemExit, match="GradChecker"):
        GradChecker(models.small_bn())
    ConvNet(models.mnist_conv(), exchange=None)   # nets without batch norm are unaffected
    GradChecker(models.mnist_conv(grad_check=True))


@pytest.mark.parametrize("C, H", [(3, 50), (1, 7), (5, 128)])
def test_bn_ref_is_the_true_gradient_of_a_linear_layer(C, H):
    # LINEAR, no dropout: the state Bprop reads IS gamma * x-hat + beta, so the reference's sequence is batch norm's true gradient
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(C * 1000 + H)
    x = rng.standard_normal((C, H)) * 3 + rng.standard_normal((C, 1))
    gamma, beta, dy = rng.uniform(0.5, 2, C), rng.standard_normal(C), rng.standard_normal((C, H))
    eps = 1e-3
    y, _, _, mb, sb = bn_ref.fprop(x, gamma, beta, np.zeros(C), np.ones(C), 0.9, eps, True)
    xt = torch.tensor(x.T, requires_grad=True)          # (H, C): torch's (batch, channels)
    gt, bt = torch.tensor(gamma, requires_grad=True), torch.tensor(beta, requires_grad=True)
    yt = torch.nn.functional.batch_norm(xt, None, None, gt, bt, training=True, eps=eps)
    np.testing.assert_allclose(yt.detach().numpy().T, y, rtol=1e-12, atol=1e-12)
    (yt * torch.tensor(dy.T)).sum().backward()
    dx, dgamma, dbeta = bn_ref.bprop(dy, y, gamma, beta, sb)
    np.testing.assert_allclose(dx, xt.grad.numpy().T, rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(dgamma * H, gt.grad.numpy(), rtol=1e-9, atol=1e-11)   # the reference's grads are means
    np.testing.assert_allclose(dbeta * H, bt.grad.numpy(), rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(mb, x.mean(axis=1)), np.testing.assert_allclose(sb, np.sqrt(x.var(axis=1) + eps))


def test_bn_ref_relu_quirk_differs_from_the_true_gradient():
    # after a ReLU the state holds 0 where the pre-activation was negative: y = -beta/gamma there, not x-hat (NOTES.md)
    rng = np.random.default_rng(3)
    C, H = 2, 64
    x = rng.standard_normal((C, H))
    gamma, beta, dy = np.array([1.5, 0.7]), np.array([0.2, -0.1]), rng.standard_normal((C, H))
    y, _, _, _, sb = bn_ref.fprop(x, gamma, beta, np.zeros(C), np.ones(C), 0.9, 1e-5, True, relu=True)
    d = np.where(y > 0, dy, 0)
    quirk = bn_ref.bprop(d, y, gamma, beta, sb)[0]
    pre = bn_ref.fprop(x, gamma, beta, np.zeros(C), np.ones(C), 0.9, 1e-5, True)[0]
    true = bn_ref.bprop(d, pre, gamma, beta, sb)[0]
    assert np.abs(quirk - true).max() > 1e-3


def test_cudamat_restatements_agree_with_each_other():
    # bn_bprop_inplace is bprop's middle (gamma = sigma = 1, beta = 0); bn_grad's dgamma is the SUM of what bprop averages
    rng = np.random.default_rng(5)
    d, act = rng.standard_normal((3, 40)), rng.standard_normal((3, 40))
    a, dg = bn_ref.bn_bprop_inplace(d, act)
    b, dg2, _ = bn_ref.bprop(d, act, np.ones(3), np.zeros(3), np.ones(3))
    np.testing.assert_allclose(a, b), np.testing.assert_allclose(dg, dg2)
    dgamma, dbeta = bn_ref.bn_grad(d, act, np.zeros(3), np.ones(3))
    np.testing.assert_allclose(dgamma / 40, dg), np.testing.assert_allclose(dbeta, d.sum(axis=1))


def test_hidden_softmax_layer_with_batch_norm_is_refused():
    text = models.small_bn().replace('  name: "fc3"\n  num_channels: 32\n  activation: RECTIFIED_LINEAR\n',
                                     '  name: "fc3"\n  num_channels: 32\n  activation: SOFTMAX\n', 1)
    assert "SOFTMAX" in text.split('name: "fc3"')[1].split("}")[0]
    with pytest.raises(SystemExit, match="only LINEAR and RECTIFIED_LINEAR"):
        ConvNet(text)


@pytest.mark.parametrize("fused", [False, True])
def test_fused_host_plans_gamma_beta_steps_into_the_batch(fused):
    # the fused host's gamma / beta SGD steps join the step's one sgd_momentum_step_multi launch: PlanFusedStep returns the step as
    # data (and advances the step counter as Optimize would); the unfused host runs the reference's Optimize
    from convnet_amd.matrix import Matrix
    net = ConvNet(models.small_bn(), fused=fused)
    for name in BN_LAYERS:
        l = net.GetLayerByName(name)
        for opt in (l.gamma_optimizer_, l.beta_optimizer_):
            assert opt.fused == fused
            g, p = Matrix(), Matrix()
            item = opt.PlanFusedStep(g, p)
            if fused:
                assert item is not None and item[0] is g and item[1] is p and opt.step_ == 1
            else:
                assert item is None and opt.step_ == 0
