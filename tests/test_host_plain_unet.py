"""Host-side logic of the plain 3D U-Net on the native path: which ConvBlock / MaxPoolBlock configurations count as
native, how the assembler classifies a chain that contains them, and what stays a torch module.  No device needed."""
import torch
import torch.nn as nn

import network


def test_conv_block_eligibility():
    assert network.ConvBlock(4, 8)._native
    assert network.ConvBlock(4, 8, dropout_op=None)._native
    assert not network.ConvBlock(4, 8, norm_op=nn.BatchNorm3d)._native
    assert not network.ConvBlock(4, 8, nonlin_op=nn.ReLU)._native
    assert not network.ConvBlock(4, 8, conv_kwargs={'kernel_size': 1})._native
    assert not network.ConvBlock(4, 8, conv_kwargs={'kernel_size': 3, 'padding': 1, 'stride': 2})._native
    assert not network.ConvBlock(4, 8, dropout_op=nn.Dropout, dropout_kwargs={'p': 0.5})._native
    assert not network.ConvBlock(4, 8, nonlin_kwargs={'negative_slope': 0.2})._native
    assert not network.ConvBlock(4, 8, norm_kwargs={'affine': True})._native
    blk = network.ConvBlock(4, 8)
    assert blk._forced_keep is None and blk._shared is False
    assert all(b._native for b in network.ConvBlockStack(4, 8, num_stacks=3).conv_blocks)


def test_max_pool_block_eligibility():
    assert network.MaxPoolBlock(4, 4)._native
    assert network.MaxPoolBlock(4, 4, pool_kwargs={'kernel_size': (2, 2, 2), 'stride': (2, 2, 2)})._native
    assert network.MaxPoolBlock(4, 4, pool_kwargs={'kernel_size': 2})._native          # the stride defaults to the kernel
    assert not network.MaxPoolBlock(4, 4, pool_op=nn.AvgPool3d)._native
    assert not network.MaxPoolBlock(4, 4, pool_kwargs={'kernel_size': 3, 'stride': 2})._native
    assert not network.MaxPoolBlock(4, 4, pool_kwargs={'kernel_size': 2, 'stride': 1})._native
    assert not network.MaxPoolBlock(4, 4, pool_kwargs={'kernel_size': 2, 'stride': 2, 'ceil_mode': True})._native
    assert not network.MaxPoolBlock(4, 4, pool_kwargs={'kernel_size': 2, 'stride': 2, 'padding': 1})._native
    assert not network.MaxPoolBlock(4, 4, pool_kwargs={'kernel_size': 2, 'stride': 2, 'return_indices': True})._native
    assert not network.MaxPoolBlock(4, 4, pool_kwargs={'kernel_size': 2, 'stride': 2, 'dilation': 2})._native


def test_plain_unet_is_a_native_chain():
    net = network.Unet(1, 3, network.generate_paired_features2(2, 4))
    chain = net._native_chain()
    assert chain is not None
    # 3 stacks of 2 + 2 stacks of 2 ConvBlocks, 2 pooling blocks, 2 transposed convs
    assert sum(isinstance(b, network.ConvBlock) for b in chain) == 10
    assert sum(isinstance(b, network.MaxPoolBlock) for b in chain) == 2
    assert sum(isinstance(b, network.ConvTrans3D) for b in chain) == 2
    assert net._in_chain is True and net._pad is False and net._linked is False and net._bn_blocks is None
    assert net._storage_dtype() == network._DEFAULT_DTYPE
    network.set_compute_dtype(net, torch.bfloat16)
    assert net._storage_dtype() == torch.bfloat16 and net._pad is False
    network.set_compute_dtype(net, torch.float16)
    assert net._storage_dtype() == torch.float16


def test_plain_unet_never_pads_even_at_padding_widths():
    net = network.Unet(1, 3, network.generate_paired_features2(2, 24))
    network.set_compute_dtype(net, torch.bfloat16)
    assert net._in_chain and net._pad is False
    res = network.ResUnet3D(2, 24, 1, 3)                    # the ResBlock chain of the same widths does
    network.set_compute_dtype(res, torch.bfloat16)
    assert res.net._pad is True and res.net._linked is True


def test_torch_switch_keeps_fp32_storage(monkeypatch):
    net = network.Unet(1, 3, network.generate_paired_features2(2, 4))
    network.set_compute_dtype(net, torch.bfloat16)
    monkeypatch.setenv("RU3D_PLAIN_BLOCKS", "torch")
    assert net._storage_dtype() == torch.float32            # torch modules behind the stem consume fp32
    monkeypatch.setenv("RU3D_PLAIN_BLOCKS", "native")
    assert net._storage_dtype() == torch.bfloat16
    res = network.ResUnet3D(2, 32, 1, 3)
    network.set_compute_dtype(res, torch.bfloat16)
    monkeypatch.setenv("RU3D_PLAIN_BLOCKS", "torch")
    assert res.net._storage_dtype() == torch.bfloat16       # no plain block in the chain: the switch does not apply


def test_chains_that_stay_torch():
    bn = network.Unet(1, 3, network.generate_paired_features2(2, 4), encode_kwargs={'norm_op': nn.BatchNorm3d})
    assert bn._native_chain() is None and bn._in_chain is False and bn._bn_blocks is None
    network.set_compute_dtype(bn, torch.bfloat16)
    assert bn._storage_dtype() == torch.float32
    avg = network.Unet(1, 3, network.generate_paired_features2(2, 4), pool_kwargs={'pool_op': nn.AvgPool3d})
    assert avg._native_chain() is None
    # BatchNorm ResBlocks around max pooling: not a BatchNorm chain either (as before)
    mix = network.Unet(1, 3, network.generate_paired_features2(2, 4), encode_block=network.ResBlockStack,
                       encode_kwargs={'norm_op': nn.BatchNorm3d}, decode_block=network.ResBlock,
                       decode_kwargs={'norm_op': nn.BatchNorm3d}, up_kwargs={'norm_op': nn.BatchNorm3d})
    assert mix._native_chain() is None and mix._bn_blocks is None


def test_mixed_chains_are_native():
    a = network.Unet(1, 2, network.generate_paired_features(2, 8), pool_block=network.ResBlock,
                     pool_kwargs={'stride': 2}, encode_block=network.ConvBlockStack, decode_block=network.ResBlock)
    b = network.Unet(1, 2, network.generate_paired_features2(2, 8), encode_block=network.ResBlockStack,
                     decode_block=network.ResBlock)
    # everything the skip links ask of encoders and pooling blocks, but plain decoders: native, and still unlinked
    c = network.Unet(1, 2, network.generate_paired_features(2, 8), pool_block=network.ResBlock,
                     pool_kwargs={'stride': 2}, encode_block=network.ResBlockStack, decode_block=network.ConvBlockStack)
    d = network.Unet(1, 2, network.generate_paired_features(2, 8), pool_block=network.ResBlock,
                     pool_kwargs={'stride': 2}, encode_block=network.ResBlockStack, decode_block=network.ConvBlock)
    for net in (c, d):
        network.set_compute_dtype(net, torch.bfloat16)
        assert net._storage_dtype() == torch.bfloat16
    for net in (a, b, c, d):
        assert net._native_chain() is not None and net._in_chain and not net._pad and not net._linked
    assert network.ResUnet3D(2, 8, 1, 2).net._linked is True       # the ResBlock net keeps its skip links


def test_rec_block_marks_its_conv_block_shared():
    rec = network.RecBlock(4, dropout_op=None)
    assert rec.conv._shared is True and rec.conv._native
    rr = network.ResRecBlock(2, 4, dropout_op=None)
    assert all(m.conv._shared for m in rr.rcnn)


def test_plain_blocks_run_on_cpu_as_torch_modules():
    torch.manual_seed(0)
    x = torch.randn(1, 2, 6, 6, 6)
    assert tuple(network.ConvBlock(2, 4)(x).shape) == (1, 4, 6, 6, 6)
    assert tuple(network.ConvBlockStack(2, 4)(x).shape) == (1, 4, 6, 6, 6)
    pooled = network.MaxPoolBlock(2, 2)(x)
    assert torch.equal(pooled, torch.nn.functional.max_pool3d(x, 2, 2))
    blk = network.ConvBlock(2, 4, dropout_op=None).eval()
    want = torch.nn.functional.leaky_relu(torch.nn.functional.instance_norm(blk.conv(x)), 0.01)
    assert torch.allclose(blk(x), want, atol=1e-6)


def test_drop_spec_and_scale_conditions():
    blk = network.ConvBlock(2, 4).train()
    assert blk._drop_spec(3) == (3, 4, 0.5)
    blk.dropout.p = 0.0
    assert blk._drop_spec(3) is None and blk._drop_scale(torch.zeros(3, 2, 2, 2, 2)) is None
    blk.dropout.p = 0.5
    blk.eval()
    assert blk._drop_spec(3) is None and blk._drop_scale(torch.zeros(3, 2, 2, 2, 2)) is None
    blk.train()
    blk._forced_keep = torch.tensor([[1.0, 0.0, 1.0, 1.0]])
    assert blk._drop_spec(1) is None
    assert blk._drop_scale(torch.zeros(1, 2, 2, 2, 2)).tolist() == [2.0, 0.0, 2.0, 2.0]


def test_new_entry_points_are_declared():
    import _native as N
    assert "ru3d_maxpool3d_fwd" in N.SIGNATURES and "ru3d_maxpool3d_bwd" in N.SIGNATURES
    assert hasattr(N.lib, "ru3d_maxpool3d_fwd") and hasattr(N.lib, "ru3d_maxpool3d_bwd")
    import _ops as ops
    assert issubclass(ops.ConvStackFn, torch.autograd.Function) and issubclass(ops.MaxPoolFn, torch.autograd.Function)
