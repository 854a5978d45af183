"""convnet_amd — MI355X-native implementation of TorontoDeepLearning/convnet's data-parallel
training hot path (conv fprop/dgrad/wgrad, pooling, response norm, FC, SGD, gradient exchange).

Layout:
  csrc/           hand-written HIP (gfx950) kernels + the C ABI (include/convnet_hip.h)
  _lib.py         ctypes binding of lib/libconvnet_hip.so
  matrix.py       class Matrix  (mirror of the reference's src/matrix.h)
  pbtxt.py        protobuf text-format reader for proto/convnet_config.proto models
  edge.py, layer.py, optimizer.py, loss_functions.py   operator classes (src/*_edge.cc, layer.cc, ...)
  convnet.py      ConvNet driver (src/convnet.cc): build/sort/alloc, Fprop/Bprop/TrainOneBatch
  data_parallel.py  RCCL gradient exchange (replaces the MPI Accumulate/Broadcast of convnet.cc:407-450)
"""
# A training step drives up to three HIP streams of its own (compute, weight gradients + optimizer steps, gradient exchange) and
# RCCL adds its internal ones.  The HIP runtime multiplexes every stream of a process onto GPU_MAX_HW_QUEUES hardware queues, and
# two streams that land on one queue run strictly one after the other.  The package leaves that setting to the environment: the
# hardware queues of a card are shared by every process on it, so raising the count is the machine's decision, not a library's.
# Measured on the MI355X: without a gradient exchange the queue count is neutral for the AlexNet step; with a 1-rank exchange on
# 4 queues the second stream shared the first one's queue (12.1 ms per step instead of 11.3).  C/C++ hosts: INTEGRATION.md §4.

__version__ = "0.1"
