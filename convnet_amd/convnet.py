"""ConvNet — mirror of src/convnet.{h,cc} for the training hot path: build the graph from a pbtxt
model, topologically sort, allocate the flat parameter / gradient buffers, Fprop / Bprop /
UpdateWeights / TrainOneBatch.

What changed relative to the reference, and why (MI355X-first):
  * Gradient exchange.  The reference D2H-copies the whole 249 MB gradient, sums it on rank 0 through
    MPI_Send/Recv, divides, and MPI_Bcasts it back (src/convnet.cc:407-450) *after* Bprop returns.
    Here every edge's gradient slice is all-reduced by RCCL (torch.distributed "nccl" backend over
    xGMI) on a communication stream the moment ComputeOuter has produced it, overlapping the rest
    of the backward pass; UpdateWeights waits per slice right before its optimizer step
    (data_parallel.GradientExchange).
  * GetLoss no longer forces a device->host sync every step (src/convnet.cc:482 -> matrix.cc:253-268):
    with ``fused=True`` the correct-count accumulates on device and is read every ``print_after``.
  * ``fused=True`` routes conv+bias+ReLU, FC+bias+ReLU, ReLU+dropout, logistic+dropout, softmax+CE-deriv+count (and its logistic
    and softmax-distribution counterparts) and the SGD step through the library's fused entry points.  ``fused=False`` issues exactly the
    reference's Matrix-call sequence (used by the parity tests and grad_check).  Which entry serves which layer is decided once, when the
    graph is built (LayerPlan); Fprop / Bprop / ComputeDeriv / GetLoss read the plan.
"""
import os
import sys
from collections import deque
from typing import Callable, NamedTuple, Optional

import torch

from . import pbtxt
from .edge import (AvgPoolEdge, ConvEdge, Edge, EdgeWithWeight, FCEdge, LocalEdge, MaxPoolEdge, ResponseNormEdge, RGBToYUVEdge,
                   UpSampleEdge)
from .layer import Layer, LinearLayer, LogisticLayer, ReLULayer, SoftmaxDistLayer, SoftmaxLayer
from .matrix import Matrix
from .optimizer import RunFusedSteps
from .trainer import TrainLoopMixin


class LayerPlan(NamedTuple):
    """Which library entries serve one layer: every per-layer choice of Fprop / Bprop / ComputeDeriv, made once by ConvNet._plan_layer
    when BuildNet has wired the graph.  An unfused net plans the reference's own sequence."""
    fuse_relu: Optional[bool]          # incoming edges' ComputeUp: None = the reference sequence, False = bias in the epilogue, True = bias and ReLU
    bn_relu: Optional[bool]            # a batch-normalised layer (else None): whether bn_fprop_act applies the ReLU in the same pass
    activate: bool                     # ApplyActivation follows: no epilogue has applied the activation
    output_entry: Optional[Callable]   # train: the state keeps the logits for this entry (activation + loss derivative + metric, ComputeDeriv)
    logistic_dropout: bool             # train: LogisticDropout instead of ApplyActivation + ApplyDropout (a logistic layer never stores its noise)
    dropout_scale: float               # Layer.TrainDropoutScale()
    down_scale: Optional[float]        # ComputeDown's post-scale: ReLU' and dropout' ride in the outgoing edges' epilogues (None: they do not)
    logistic_deriv: bool               # LogisticDerivScaled instead of ApplyDerivativeofDropout + ApplyDerivativeOfActivation


def _zero_storage(m):
    """Zeroes the device storage a matrix owns; one that owns none (a stand-in that only records allocations) has nothing to zero."""
    t = getattr(m, "_t", None)
    if t is not None:
        t.zero_()


class ConvNet(TrainLoopMixin):
    def __init__(self, model, fused=False, process_id=0, num_processes=1, verbose=False, exchange=None, overlap_update=None,
                 overlap_wgrad=None):
        """``model``: path to a pbtxt file, pbtxt text, or a parsed pbtxt.Model.
        ``overlap_update`` (default off): inside TrainOneBatch each edge's optimizer step is enqueued on a second
        HIP stream as soon as that edge's wgrad + dgrad (and, data-parallel, its gradient bucket's all-reduce)
        are done.  Same arithmetic as the reference's serial UpdateWeights (bit-identical, tested).  Measured on
        one MI355X it is throughput-neutral (18.34 vs 18.36 ms/step): the co-running HBM-bound update kernels take
        CU slots from the MFMA kernels and slow them by what they save, so it stays opt-in.
        ``overlap_wgrad`` (default off): inside TrainOneBatch every edge's ComputeOuter (weight gradient, matrix-pipe bound) is
        enqueued on the second stream, ordered after the derivative it reads; the main stream goes straight on to the edge's
        ComputeDown and the next layers' backward (pool / response-norm undo are HBM-bound and can share the chip with it).
        The optimizer step (on either stream) and the gradient exchange are ordered behind it.  Same arithmetic."""
        self.verbose = verbose
        self.fused = fused
        self.overlap_update_ = bool(overlap_update)
        self.overlap_wgrad_ = bool(overlap_wgrad)
        # Where a conv edge's weight gradient joins the second stream.  "before": as soon as the edge's output derivative is final, so it
        # runs beside the edge's own ComputeDown; "after": behind that ComputeDown, beside what follows it on the main stream (the previous
        # layer's response-norm / pool undo).  Same arithmetic; which pairing is faster is a property of the kernels of the day: round 3
        # measured "after" 0.08 ms ahead; with round 4's kernels (faster gather-GEMMs, the 2 x 2-block pool undo) "before" is 0.25 ms ahead
        # (10.98-11.00 vs 11.23-11.28 ms, same call, profiles/r04_kernel_experiments.md §4).  CONVNET_WGRAD_ORDER overrides (A/B runs).
        self.wgrad_order_ = os.environ.get("CONVNET_WGRAD_ORDER", "before")
        self.side_stream_ = None
        self._pending_updates = []     # [(edge, event on the main stream after its dgrad, held back?)]
        self._in_train_step = False
        self.process_id_ = process_id
        self.num_processes_ = num_processes
        self.is_root_ = process_id == 0
        self.exchange_ = exchange
        if isinstance(model, pbtxt.Model):
            self.model_ = model
        elif "\n" in model or "{" in model:
            self.model_ = pbtxt.parse(model)
        else:
            self.model_ = pbtxt.read(model)
        m = self.model_
        # default optimizers for weights/biases whose optimizer is not specified (src/convnet.cc:36-50)
        for e in m.edge:
            if Edge.HasParameters(e):
                w_opt = m.default_weight_optimizer.copy()
                w_opt.MergeFrom(e.weight_optimizer)
                e.mutable("weight_optimizer").CopyFrom(w_opt)
                if not e.has_no_bias:
                    b_opt = m.default_bias_optimizer.copy()
                    b_opt.MergeFrom(e.bias_optimizer)
                    e.mutable("bias_optimizer").CopyFrom(b_opt)
        # ... and for batch-normalised layers (src/convnet.cc:56-64), quirk included: beta's own block is merged into the GAMMA
        # config's copy (which is then unused), so beta always runs the plain default bias optimizer
        for l in m.layer:
            if l.batch_normalize:
                w_opt = m.default_weight_optimizer.copy()
                w_opt.MergeFrom(l.gamma_optimizer)
                l.mutable("gamma_optimizer").CopyFrom(w_opt)
                b_opt = m.default_bias_optimizer.copy()
                w_opt.MergeFrom(l.beta_optimizer)
                l.mutable("beta_optimizer").CopyFrom(b_opt)
        Matrix.InitRandom(m.seed + process_id)   # src/convnet.cc:67
        self.model_name_ = m.name
        self.layers_, self.edges_ = [], []
        self.input_layers_, self.output_layers_, self.data_layers_ = [], [], []
        self.batch_size_ = 0
        self.current_iter_ = 0
        self.parameters_, self.grad_parameters_, self.history_ = Matrix(), Matrix(), Matrix()
        self.second_history_ = Matrix()   # Adagrad / RMSProp second moments, flat like history_; allocated only if an edge optimizer keeps one
        self.edge_slices_ = {}   # edge -> (offset, length) in the flat buffers
        self.train_dataset_ = None
        self.train_dataset_config_ = self.valid_dataset_config_ = None   # the DatasetConfigs of SetupDataset(train_pbtxt, val_pbtxt)
        self.correct_accum_ = None
        self._logits_pending = set()   # output layers whose state still holds logits (fused softmax / logistic / softmax-distribution)
        self._bn_steps = []            # fused host: the gamma / beta SGD steps planned during Bprop, run with the edges' batch
        self.BuildNet()
        if exchange is not None and any(l.UseBatchNormalization() for l in self.layers_):
            # the reference keeps gamma / beta per replica and steps them inside Bprop, before any exchange: P x (B/P) != 1 x B
            raise SystemExit("batch_normalize is not supported with a gradient exchange (data-parallel training)")

    def log(self, *a):
        if self.verbose:
            print(*a, file=sys.stderr)

    # ---- graph: src/convnet.cc:150-242 ---------------------------------------------------------------
    def BuildNet(self):
        m = self.model_
        self.layers_ = [Layer.ChooseLayerClass(l) for l in m.layer]
        self.edges_ = [Edge.ChooseEdgeClass(e) for e in m.edge]
        by_name = {e.GetName(): e for e in self.edges_}
        for e in self.edges_:
            if e.IsTied():
                e.SetTiedTo(by_name[e.GetTiedEdgeName()])
        for l in self.layers_:
            for e in self.edges_:
                if l.GetName() == e.GetSourceName():
                    l.AddOutgoing(e)
                    e.SetSource(l)
                    e.SetInputChannels(l.GetNumChannels(e.GetSourceSliceName()))
                if l.GetName() == e.GetDestName():
                    l.AddIncoming(e)
                    e.SetDest(l)
                    e.SetOutputChannels(l.GetNumChannels(e.GetDestSliceName()))
        self.Sort()
        # the edges, the layers and their optimizers all switch on ``fused`` (fused host: the plain steps, a batch-normalised layer's
        # gamma / beta steps included, are planned into the step's one multi launch, PlanFusedStep)
        for x in (*self.edges_, *self.layers_):
            x.fused = self.fused
            for opt in (getattr(x, n, None) for n in ("weight_optimizer_", "bias_optimizer_", "gamma_optimizer_", "beta_optimizer_")):
                if opt is not None:
                    opt.fused = self.fused
        for l in self.layers_:
            if l.UseBatchNormalization():
                self._check_batch_norm(l)
            self._check_slices(l)
            self._check_resample_edges(l)
            self._check_gaussian_dropout(l)
            if not l.incoming_edge_:
                self.input_layers_.append(l)
                self.data_layers_.append(l)
            if not l.outgoing_edge_:
                self.output_layers_.append(l)
                self.data_layers_.append(l)
        for l in self.layers_:
            if l.IsInput():
                y, x, t = l.GetSizeY(), l.GetSizeX(), l.GetSizeT()
                if y <= 0:
                    y = m.patch_size
                if x <= 0:
                    x = m.patch_size
                if t <= 0:
                    t = 1
            else:
                e0 = l.incoming_edge_[0]
                y, x, t = e0.GetNumModulesY(), e0.GetNumModulesX(), e0.GetNumModulesT()
            l.SetSize(y, x, t)
            if t > 1 and l.UseBatchNormalization():
                # the (-1, C) view of the state groups by channel only for one frame (time is the outermost index)
                raise SystemExit(f"batch_normalize on layer {l.GetName()}: not supported on a layer with image_size_t > 1 ({t} frames)")
            if t > 1 and l.HasSlices():
                # the reference cuts pixels * T * channels contiguous columns, which is no channel range of a time-major tensor
                raise SystemExit(f"layer_slice on layer {l.GetName()}: not supported on a layer with image_size_t > 1 ({t} frames): "
                                 "time is the outermost index, so a channel range is not one column range")
            self.log(f"Layer {l.GetName()}: {y}x{x}")
            for e in l.outgoing_edge_:
                e.SetImageSize(y, x, t)
        self.PlanLayers()

    def PlanLayers(self):
        """Every layer's LayerPlan.  BuildNet ends with it; whoever changes a built graph by hand (a test) calls it again."""
        self.plan_ = {l: self._plan_layer(l) for l in self.layers_}
        # Beside the plan: the hidden Gaussian-dropout layers whose backward pass must leave the state as the reference does, divided by
        # the noise again, because something reads it afterwards — batch normalisation's derivative, or the undo of a max-pool or
        # response-norm edge INTO the layer (both compare or combine with their output's state).  The unfused sequence restores it
        # always; the fused undo only here, and elsewhere leaves the state alone
        self.gaussian_restore_ = {l for l in self.layers_ if l.gaussian_dropout_ and not l.IsInput() and (
            not l.FusedGaussianDropout() or l.UseBatchNormalization()
            or any(isinstance(e, (MaxPoolEdge, ResponseNormEdge)) for e in l.incoming_edge_))}
        # the metric accumulates on the device (GetLoss returns None) only for one output on a fused output entry: the counter is one number
        self.metric_on_device_ = len(self.output_layers_) == 1 and self.plan_[self.output_layers_[0]].output_entry is not None

    def _fused_down_scale(self, l):
        return self.plan_[l].down_scale   # the ComputeDown post-scale planned for layer l, or None (the tests ask by layer)

    def _plan_layer(self, l):
        """The LayerPlan of layer l, from what BuildNet has fixed: the layer's class and dropout, its edge lists, the edges' classes,
        bias kinds and block_backprop, the number of output layers.  Also sets the verdict on the max-pool mask pair on l's incoming
        max-pool edges (the edges' own ``fused`` stays a live switch: MaxPoolEdge.MaskEligible)."""
        fused, hidden = self.fused, not l.IsInput() and not l.IsOutput()
        bn, logistic, scale = l.UseBatchNormalization(), isinstance(l, LogisticLayer), l.TrainDropoutScale()
        for e in l.incoming_edge_:
            if isinstance(e, MaxPoolEdge):
                # the mask pair equals the reference's MaxPoolUndo only if backprop sees the raw maxima (edge.MaxPoolEdge)
                e.mask_legal_ = l.dropprob_ == 0 and type(l) in (LinearLayer, ReLULayer)
        # forward.  The incoming edges' epilogues take the bias, and the ReLU unless batch normalisation sits in between, when every one of
        # them is the only writer of its destination — the whole layer, or a slice of a layer whose written slices are all of it; a
        # sigmoid is a pass of its own, a softmax layer takes the reference's calls.  All or nothing per layer
        fuse_up = (fused and self._each_alone_and_all_of(l, [e.GetDestSliceName() for e in l.incoming_edge_])
                   and not isinstance(l, SoftmaxLayer) and all(e.CanFuseUp(l) for e in l.incoming_edge_))
        activate = not fused if bn else not l.IsInput() and (not fuse_up or logistic)
        # output: softmax always; logistic and softmax-distribution for a single output without dropout whose loss and metric are the
        # ones the entry computes.  Anything else runs the reference's calls
        entry = None
        if fused and l.IsOutput() and not l.IsInput():
            single = len(self.output_layers_) == 1 and l.dropprob_ <= 0
            if type(l) is SoftmaxLayer:
                entry = Matrix.SoftmaxCEGradCorrect
            elif single and logistic and (l.loss_function_, l.performance_metric_) == ("CROSS_ENTROPY_BINARY", "CLASSIFICATION_BINARY"):
                entry = Matrix.LogisticCEGradCorrect
            elif single and isinstance(l, SoftmaxDistLayer) and l.loss_function_ == l.performance_metric_ == "CROSS_ENTROPY_MULTINOMIAL_DISTRIBUTED":
                entry = Matrix.SoftmaxDistCEGrad
        # backward.  The reference applies dropout' and ReLU' after ALL outgoing edges have accumulated (src/convnet.cc:390-404), so they
        # ride in the ComputeDown epilogues only where every edge is the only reader of what it reads — the whole layer, or a slice of a
        # layer whose read slices are all of it; a max-pool undo masks but does not scale
        # A Gaussian-dropout layer takes none of the three dropout fusions below: its derivative is multiplied by the noise and its
        # activation's derivative taken at state / noise (Layer.ApplyDerivativeofGaussianDropout; a fused one stores no noise, so
        # store_dropout_noise_ says nothing about it)
        gaussian = l.gaussian_dropout_
        down_scale = None
        if (fused and hidden and l.is_relu and not gaussian
                and self._each_alone_and_all_of(l, [e.GetSourceSliceName() for e in l.outgoing_edge_])):
            if all(e.can_fuse_mask and not e.IsBackPropBlocked() and not l.store_dropout_noise_
                   and not (isinstance(e, MaxPoolEdge) and scale != 1.0) for e in l.outgoing_edge_):
                down_scale = scale
        return LayerPlan(fuse_relu=(l.is_relu and not bn) if fuse_up else None, bn_relu=(fused and l.is_relu) if bn else None,
                         activate=activate, output_entry=entry,
                         logistic_dropout=fused and logistic and not l.IsInput() and l.dropprob_ > 0 and not gaussian,
                         dropout_scale=scale, down_scale=down_scale, logistic_deriv=fused and logistic and hidden and not gaussian)

    @staticmethod
    def _each_alone_and_all_of(l, slice_names):
        """Whether the edges that name these slices of layer l ("" = the whole layer) each have theirs to themselves and together touch
        every channel of l: one edge on the whole layer, or one edge per slice of a layer that has no channels outside its slices."""
        if slice_names == [""]:
            return True
        if not slice_names:
            return False
        return (len(set(slice_names)) == len(slice_names) and set(slice_names) == set(l.slice_channels_)
                and l.GetNumChannels() == sum(l.slice_channels_.values()))

    @staticmethod
    def _check_slices(l):
        """The supported set of sliced layers; anything else stops with the reason."""
        name = l.GetName()
        for what, edges, get in (("read", l.outgoing_edge_, Edge.GetSourceSliceName), ("written", l.incoming_edge_, Edge.GetDestSliceName)):
            whole = [e.GetName() for e in edges if not get(e)]
            part = [e.GetName() for e in edges if get(e)]
            if whole and part:
                # the whole-layer flag and the slice flags are independent (src/layer.cc:307-327): the second writer overwrites where it
                # should add, and in Bprop the second reader's gradient replaces the first's
                raise SystemExit(f"layer_slice on layer {name}: the layer is {what} both whole (edge {whole[0]}) and by slice (edge {part[0]}); "
                                 "their add-or-overwrite flags are independent, so one would overwrite what the other has written")
        if l.UseBatchNormalization():
            if l.HasSlices():
                raise SystemExit(f"batch_normalize on layer {name}: not supported on a layer with slices")
            for e in l.incoming_edge_:
                if e.GetSourceSliceName():
                    raise SystemExit(f"batch_normalize on layer {name}: not supported on a layer fed from a slice (edge {e.GetName()})")

    @staticmethod
    def _check_resample_edges(l):
        """What an UPSAMPLE or RGBTOYUV edge out of layer l cannot be; each stops with its reason."""
        for e in l.outgoing_edge_:
            if isinstance(e, RGBToYUVEdge) and l.incoming_edge_ and not e.IsBackPropBlocked():
                # (an input layer takes no derivative, src/convnet.cc:370; nor does anything behind a blocked edge)
                raise SystemExit(f"Error: Edge {e.GetName()}: RGBTOYUV has no backward pass (\"RGBtoYUV backprop Not implemented.\"), and its "
                                 f"source layer {l.GetName()} needs a derivative: read an input layer, or set block_backprop on the edge.")
            if isinstance(e, UpSampleEdge) and l.incoming_edge_ and not e.IsBackPropBlocked():
                others = [f.GetName() for f in l.outgoing_edge_
                          if f is not e and not f.IsBackPropBlocked() and f.GetSourceSliceName() == e.GetSourceSliceName()]
                if others:
                    # UpSampleEdge::ComputeDown ignores `overwrite` (src/upsample_edge.cc:30-34)
                    raise SystemExit(f"Error: Edge {e.GetName()}: the backward pass of UPSAMPLE overwrites the derivative of its source layer "
                                     f"{l.GetName()}, which edge {others[0]} also back-propagates into: its part would be lost.  Give the "
                                     "UPSAMPLE edge a source layer of its own, or set block_backprop on one of the two.")

    @staticmethod
    def _check_gaussian_dropout(l):
        """Where a Gaussian-dropout layer can stand (Layer.__init__ has checked dropprob); anything else stops with the
        reason."""
        if not l.gaussian_dropout_:
            return
        name = l.GetName()
        if l.IsOutput():
            raise SystemExit(f"gaussian_dropout on layer {name}: not supported on an output layer (the prediction that is compared with "
                             "the target would be the noised one)")
        if type(l) not in (LinearLayer, ReLULayer, LogisticLayer):
            raise SystemExit(f"gaussian_dropout on layer {name}: only LINEAR, RECTIFIED_LINEAR and LOGISTIC activations are supported")

    @staticmethod
    def _check_batch_norm(l):
        """The supported set of batch-normalised layers; anything else stops with the reason."""
        name = l.GetName()
        if l.IsInput() or l.IsOutput():
            raise SystemExit(f"batch_normalize on layer {name}: input and output layers cannot be batch-normalised")
        if type(l) not in (LinearLayer, ReLULayer):
            raise SystemExit(f"batch_normalize on layer {name}: only LINEAR and RECTIFIED_LINEAR activations are supported")
        for e in l.incoming_edge_:
            if isinstance(e, (MaxPoolEdge, ResponseNormEdge)):
                # their undo reads this layer's output state, which batch normalisation has overwritten (the reference then routes
                # almost no gradient)
                raise SystemExit(f"batch_normalize on layer {name}: not supported behind a {e.__class__.__name__} (edge {e.GetName()})")
            if not isinstance(e, (FCEdge, ConvEdge, LocalEdge, AvgPoolEdge)):
                raise SystemExit(f"batch_normalize on layer {name}: edge {e.GetName()} ({e.__class__.__name__}) is not supported")

    def Sort(self):
        # breadth-first topological sort, src/convnet.cc:312-353
        L, S = [], deque(l for l in self.layers_ if l.IsInput())
        if not S:
            raise SystemExit("Error: No layer is set to be input!")
        while S:
            n = S.popleft()
            L.append(n)
            for e in n.outgoing_edge_:
                e.SetMark()
                mm = e.GetDest()
                if mm is None:
                    raise SystemExit(f"Edge {e.GetName()} has no destination layer")
                if all(f.HasMark() for f in mm.incoming_edge_):
                    S.append(mm)
        if not all(f.HasMark() for f in self.edges_):
            raise SystemExit("Error : Network has loop(s)!")
        self.layers_ = L

    def GetLayerByName(self, name):
        for l in self.layers_:
            if l.GetName() == name:
                return l
        raise SystemExit(f"Error: No layer called {name}")

    def GetEdgeByName(self, name):
        for e in self.edges_:
            if e.GetName() == name:
                return e
        raise SystemExit(f"Error: No edge called {name}")

    # ---- memory: src/convnet.cc:266-310 -----------------------------------------------------------------
    def SetBatchsize(self, batch_size):
        self.batch_size_ = batch_size

    def AllocateMemory(self, fprop_only=False):
        self.AllocateLayerMemory()
        self.AllocateEdgeMemory(fprop_only)
        if self.fused:
            self.correct_accum_ = Matrix()
            self.correct_accum_.AllocateGPUMemory(1, 1, "correct count")
            self.correct_accum_.Set(0.0)

    def AllocateLayerMemory(self):
        for l in self.layers_:
            l.AllocateMemory(self.batch_size_)

    def AllocateEdgeMemory(self, fprop_only):
        total, usage = 0, {}
        for e in self.edges_:
            mem = e.GetParameterMemoryRequirement()
            usage[e] = mem
            total += ((mem + 127) // 128) * 128   # 128-float aligned slices (src/convnet.cc:279)
        self.parameters_.AllocateGPUMemory(1, total, "parameters")
        # The padding between the 128-float slices is written by nobody: what the allocator left there (NaN bit patterns, after byte or
        # integer tensors) would stay in the flat buffers for good.  Their storage is handed out zeroed (the owner's job: no library call).
        _zero_storage(self.parameters_)
        if not fprop_only:
            self.grad_parameters_.AllocateGPUMemory(1, total, "grad parameters")
            self.grad_parameters_.Set(0.0)
            self.history_.AllocateGPUMemory(1, total, "optimizer history")   # flat, same layout
            _zero_storage(self.history_)
            second = any(o is not None and o.NeedsSecondHistory() for e in self.edges_ if isinstance(e, EdgeWithWeight)
                         for o in (e.weight_optimizer_, e.bias_optimizer_))
            if second:
                self.second_history_.AllocateGPUMemory(1, total, "optimizer second-moment history")
                _zero_storage(self.second_history_)
        offset = 0
        for e in self.edges_:
            mem = usage[e]
            if mem == 0:
                continue
            s = Matrix()
            self.parameters_.GetSlice(s, offset, offset + mem)
            e.SetMemory(s)
            if not fprop_only:
                g, h, h2 = Matrix(), Matrix(), None
                self.grad_parameters_.GetSlice(g, offset, offset + mem)
                self.history_.GetSlice(h, offset, offset + mem)
                if second:
                    h2 = Matrix()
                    self.second_history_.GetSlice(h2, offset, offset + mem)
                e.SetGradMemory(g, h, h2)
            self.edge_slices_[e] = (offset, mem)
            offset += ((mem + 127) // 128) * 128
        if self.is_root_ or self.exchange_ is None:
            for e in self.edges_:
                e.Initialize()
        if self.exchange_ is not None:
            self.exchange_.Broadcast(self.parameters_)   # src/convnet.cc:309
            if not fprop_only:
                self.exchange_.Register(self)

    def NumParameters(self):
        return sum(n for _, n in self.edge_slices_.values())

    # ---- fprop / bprop: src/convnet.cc:355-405 ---------------------------------------------------------
    def Fprop(self, train):
        for l in self.layers_:
            p = self.plan_[l]
            for e in l.incoming_edge_:
                overwrite = l.AddOrOverwriteState(e.GetDestSliceName())
                e.ComputeUp(e.GetSource().GetState(e.GetSourceSliceName()), l.GetState(e.GetDestSliceName()), overwrite, train,
                            fuse_relu=p.fuse_relu)
            if p.bn_relu is not None:
                l.ApplyBatchNormalization(train, relu=p.bn_relu)   # src/convnet.cc:382-384
            if train and p.output_entry is not None:
                self._logits_pending.add(l)
            elif train and p.logistic_dropout:
                l.GetState().LogisticDropout(l.dropprob_, p.dropout_scale)
                continue
            elif train and l.FusedGaussianDropout():
                # the activation rides along unless an epilogue or bn_fprop_act has applied it (an input layer has none to apply)
                l.ApplyGaussianDropout(l.gaussian_act if p.activate else 0)
                continue
            elif p.activate:
                l.ApplyActivation()
            l.ApplyDropout(train)

    def _bprop_edge(self, output, input, edge, fuse_mask=None):
        # ConvNet::Bprop(output, input, edge), src/convnet.cc:362-375
        if edge.IsBackPropBlocked():
            return
        side = self._in_train_step and self.side_stream_ is not None
        if side and isinstance(edge, ConvEdge) and any(held for _, _, held in self._pending_updates):
            # the FC updates held back so far start now, beside this conv edge's MFMA-bound backward
            now = torch.cuda.Event()
            now.record(torch.cuda.current_stream())
            self._pending_updates = [(e, now, False) for e, _, _ in self._pending_updates]
            self._flush_updates(final=False)
        # The gradient slice belongs to the OWNER of the weights: an edge tied to another one (tied_to) accumulates into its
        # owner's slice (edge_with_weight.cc:66-90), so the slice is final only when the last sharing edge has added its part —
        # whichever of them comes last in backward order.
        owner = edge.tied_edge_ if edge.IsTied() else edge
        # the edge works on the slices it names ("" = the whole layer): src/convnet.cc:364-367
        src_slice, dst_slice = edge.GetSourceSliceName(), edge.GetDestSliceName()
        input_state, output_state = input.GetState(src_slice), output.GetState(dst_slice)
        output_deriv = output.GetDeriv(dst_slice)

        def dgrad():
            if not input.IsInput():
                overwrite = input.AddOrOverwriteDeriv(src_slice)
                edge.ComputeDown(output_deriv, input_state, output_state, input.GetDeriv(src_slice), overwrite, fuse_mask=fuse_mask)

        if side and self.overlap_wgrad_ and isinstance(edge, EdgeWithWeight):
            # weight gradient on the second stream, behind everything enqueued so far (the derivative it reads); the all-reduce of
            # a completed slice is posted from that stream too, so its `ready` event covers the wgrad.  ComputeOuter reads the
            # source layer's state and the destination's derivative; ComputeDown writes the SOURCE's derivative: either order of the
            # two is legal, and nothing later in this step writes what the weight gradient reads.
            late = self.wgrad_order_ == "after" and isinstance(edge, ConvEdge)
            if late:
                dgrad()
            here = torch.cuda.Event()
            here.record(torch.cuda.current_stream())
            self.side_stream_.wait_event(here)
            with Matrix.OnStream(self.side_stream_):
                edge.ComputeOuter(input_state, output_deriv)
                complete = isinstance(owner, EdgeWithWeight) and owner.GetNumGradsReceived() >= owner.num_shares_
                if self.exchange_ is not None and owner in self.edge_slices_ and complete:
                    self.exchange_.GradReady(owner)
            if not late:
                dgrad()
        else:
            edge.ComputeOuter(input_state, output_deriv)
            complete = isinstance(owner, EdgeWithWeight) and owner.GetNumGradsReceived() >= owner.num_shares_
            if self.exchange_ is not None and owner in self.edge_slices_ and complete:
                self.exchange_.GradReady(owner)     # the slice is final: start its all-reduce
            dgrad()
        if side and self.overlap_update_ and isinstance(owner, EdgeWithWeight) and complete:
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream())   # wgrad AND dgrad (which reads the weights) are enqueued
            # An FC edge's backward at batch <= a few hundred is itself HBM-bound (it streams the weight matrix
            # three times), so running its update beside it gains nothing: hold it until a conv edge's backward
            # (MFMA-bound) begins.  Conv updates are small and start at once.
            # (Weights shared by tied edges are also READ by the sharers' ComputeDown: every sharer's dgrad precedes the
            # completing ComputeOuter in program order except the completing edge's own, enqueued just above — so `ev` covers all.)
            self._pending_updates.append((owner, ev, isinstance(owner, FCEdge)))
            self._flush_updates(final=False)

    def _flush_updates(self, final):
        """Enqueue on the side stream the optimizer step of every pending edge whose gradient is final."""
        keep = []
        for edge, ev, held in self._pending_updates:
            if held and not final:
                keep.append((edge, ev, held))
                continue
            bucket_ev = None
            if self.exchange_ is not None and edge in self.edge_slices_:
                state = self.exchange_.BucketState(edge)
                if state == "pending":
                    if final:
                        raise RuntimeError(f"gradient bucket of {edge.GetName()} was never exchanged")
                    keep.append((edge, ev, held))
                    continue
                bucket_ev = state
            self.side_stream_.wait_event(ev)
            if bucket_ev is not None and not hasattr(bucket_ev, "wait_library_stream"):
                self.side_stream_.wait_event(bucket_ev)
            with Matrix.OnStream(self.side_stream_):
                if hasattr(bucket_ev, "wait_library_stream"):
                    bucket_ev.wait_library_stream()      # exchange through the library's own entries: it holds the done-events
                edge.UpdateWeights()
        self._pending_updates = keep

    def Bprop(self):
        for l in reversed(self.layers_):
            p = self.plan_[l]
            for e in l.outgoing_edge_:
                self._bprop_edge(e.GetDest(), l, e, fuse_mask=p.down_scale)
            if l in self.gaussian_restore_ and self._in_train_step and self.side_stream_ is not None and self.overlap_wgrad_:
                # the state is divided by the noise in place, and the weight gradients of this layer's outgoing edges read it on the
                # side stream: order the rewrite after them (as for batch normalisation below)
                ev = torch.cuda.Event()
                ev.record(self.side_stream_)
                torch.cuda.current_stream().wait_event(ev)
            if p.logistic_deriv:
                l.GetDeriv().LogisticDerivScaled(l.GetState(), p.dropout_scale)   # dropout' and logistic' in one pass
            elif l.FusedGaussianDropout():
                if not l.IsInput():   # (an input layer takes no derivative; a Gaussian layer is never an output)
                    l.ApplyDerivativeofGaussianDropout(l in self.gaussian_restore_)   # dropout' and the activation's derivative in one pass
            elif p.down_scale is None:   # else dropout' and ReLU' were applied by the edge's epilogue
                l.ApplyDerivativeofDropout()
                if not l.IsInput() and not l.IsOutput():
                    l.ApplyDerivativeOfActivation()
            if l.UseBatchNormalization():
                # src/convnet.cc:401-403
                if not self.fused and self._in_train_step and self.side_stream_ is not None and self.overlap_wgrad_:
                    # the unfused sequence rewrites the state in place (recover y, restore), and the weight gradients of this layer's
                    # outgoing edges read that state on the side stream: order the rewrite after them
                    ev = torch.cuda.Event()
                    ev.record(self.side_stream_)
                    torch.cuda.current_stream().wait_event(ev)
                l.ApplyDerivativeofBatchNormalization(self._bn_steps if (self.fused and self._in_train_step) else None)

    def ComputeDeriv(self):
        for l in self.output_layers_:
            if l in self._logits_pending:
                self._logits_pending.discard(l)
                self.plan_[l].output_entry(l.GetState(), l.GetData(), l.GetState(), l.GetDeriv(), self.correct_accum_, l.loss_function_weight_)
            else:
                l.ComputeDeriv()

    def GetLoss(self):
        """Per-output-layer performance metric (src/convnet.cc:456-461).  In fused mode a softmax output's correct count (a
        logistic output's normalised correct count, a softmax-distribution output's cross entropy) accumulates on device (no
        per-step sync; ReadCorrectCount) and GetLoss returns None — unless some output layer did not take a fused output path
        (e.g. a SQUARED_ERROR linear output) or there are several outputs: the on-device counter is one number, so those nets
        report per layer through the reference's own call, like the unfused path."""
        return None if self.metric_on_device_ else [l.GetPerformanceMetric() for l in self.output_layers_]

    def TimestampModel(self):
        """ConvNet::TimestampModel (src/convnet.cc:830-838): stamp the run — checkpoints go to <dir>/<name>_<timestamp>.h5 — append
        the stamp to the model, write the stamped model as <dir>/<name>_<timestamp>.pbtxt and name the two log files."""
        import time
        ts = time.strftime("%Y%m%d%H%M%S")
        while ts in self.model_.timestamp:   # a resume within the same second must not reuse the name
            ts += "_"
        self.model_.timestamp.append(ts)
        fname = os.path.join(self.model_.checkpoint_dir, f"{self.model_.name}_{ts}")
        if self.model_.checkpoint_dir:
            os.makedirs(self.model_.checkpoint_dir, exist_ok=True)
            pbtxt.write(fname + ".pbtxt", self.model_)
        self.log_file_ = fname + "_train.log"
        self.val_log_file_ = fname + "_valid.log"
        return ts

    def ReadCorrectCount(self, reset=True):
        """Fused mode: the output layer's metric summed since the last read (one D2H sync)."""
        v = float(self.correct_accum_.ToNumpy().reshape(-1)[0])
        if reset:
            self.correct_accum_.Set(0.0)
        return v

    # ---- update: src/convnet.cc:440-450 -------------------------------------------------------------------
    def UpdateWeights(self):
        bn_steps, self._bn_steps = self._bn_steps, []
        if self._in_train_step and self.side_stream_ is not None:
            if self.overlap_update_:
                # every edge went through _bprop_edge: drain what is still waiting for its bucket, then make the
                # main stream (next Fprop reads the weights) wait for the side stream
                self._flush_updates(final=True)
            done = torch.cuda.Event()
            done.record(self.side_stream_)
            torch.cuda.current_stream().wait_event(done)   # weight gradients (and side-stream updates) are in
            if self.overlap_update_:
                RunFusedSteps(bn_steps)
                return
        # fused host: the plain SGD steps of every edge (AlexNet: five convolution banks and eight biases) leave as ONE launch behind the loop
        batch = list(bn_steps) if self.fused else None   # (+ the batch-norm gamma / beta steps planned during Bprop)
        for e in self.edges_:
            if e.IsBackPropBlocked():
                continue
            if self.exchange_ is not None and e in self.edge_slices_:
                self.exchange_.WaitFor(e)       # the averaged gradient slice has arrived
            if batch is not None and isinstance(e, EdgeWithWeight):
                e.UpdateWeights(batch)
            else:
                e.UpdateWeights()
        if batch:
            RunFusedSteps(batch)

    # ---- data -------------------------------------------------------------------------------------------
    def SetupDataset(self, dataset, val_data_config_file=""):
        """A handler object (anything with the DataHandler protocol), or — ConvNet::SetupDataset (src/convnet.cc:495-536) — the path of
        the training set's DatasetConfig pbtxt and, optionally, the validation set's."""
        if not isinstance(dataset, str):
            self.train_dataset_ = dataset
            self.batch_size_ = dataset.GetBatchSize()
            return
        # The reference keeps the two configs in model_.train_dataset / valid_dataset; pbtxt.Model has no such fields (the model
        # files' schema stays as it is), so they live on the net.
        if dataset:
            self.train_dataset_config_ = pbtxt.read(dataset, pbtxt.DatasetConfig)
        if val_data_config_file:
            self.valid_dataset_config_ = pbtxt.read(val_data_config_file, pbtxt.DatasetConfig)
        if self.train_dataset_config_ is None:
            raise SystemExit("Error: No training set provided.")
        if self.valid_dataset_config_ is None:
            self.log("Warning: No validation set provided.")
        self.train_dataset_ = self._build_data_handler(self.train_dataset_config_)
        self.SetBatchsize(self.train_dataset_.GetBatchSize())
        self.log("Training data set size", self.train_dataset_.GetDataSetSize())
        if self.valid_dataset_config_ is not None:
            self.val_dataset_ = self._build_data_handler(self.valid_dataset_config_)
            self.log("Validation data set size", self.val_dataset_.GetDataSetSize())

    def _build_data_handler(self, config):
        from .datahandler import DataHandler
        dh = DataHandler(config, seed=self.model_.seed + self.process_id_)
        by_name = {l.GetName(): l for l in self.data_layers_}
        for name, st in dh.streams_.items():
            l = by_name.get(name)
            if l is None:
                raise SystemExit(f"Data stream for layer {name}: the model has no input or output layer of that name.")
            if l.IsInput():
                want = l.GetSizeY() * l.GetSizeX() * l.GetSizeT() * l.GetNumChannels()
                if st.StagedDims() != want:
                    raise SystemExit(f"Data stream for layer {name}: the stream stages {st.StagedDims()} values per case "
                                     f"(rows of {st.GetDims()}, cropped to gpu_image_size), the layer holds {want}.")
        dh.SetInputLayers([l.GetName() for l in self.data_layers_ if l.IsInput()])
        return dh

    def GetBatch(self, dataset):
        dataset.GetBatch(self.data_layers_)

    def TrainOneBatch(self):
        # src/convnet.cc:475-485
        for l in self.layers_:
            l.ResetAddOrOverwrite()
        for e in self.edges_:
            e.NotifyStart()
        for l in self.layers_:
            l.NotifyStart()
        if self.exchange_ is not None:
            self.exchange_.StartStep()
        if (self.overlap_update_ or self.overlap_wgrad_) and self.side_stream_ is None and torch.cuda.is_available():
            self.side_stream_ = Matrix.SharedStream("side")
        self.GetBatch(self.train_dataset_)
        self.Fprop(True)
        self.ComputeDeriv()
        error = self.GetLoss()
        self._in_train_step = True
        try:
            self.Bprop()
            self.UpdateWeights()
        finally:
            self._in_train_step = False
        self.current_iter_ += 1
        return error

    # ---- checkpoint / resume: src/convnet.cc:659-684,737-751 ------------------------------------------------------------
    def ReduceLearningRate(self, factor):
        # src/convnet.cc:826-830
        for e in self.edges_:
            if isinstance(e, EdgeWithWeight):
                e.ReduceLearningRate(factor)

    def GetCheckpointFilename(self):
        # src/convnet.cc:651-657: <checkpoint_dir>/<name>_<timestamp>.h5
        m = self.model_
        ts = m.timestamp[-1] if m.timestamp else ""
        return os.path.join(m.checkpoint_dir, f"{m.name}_{ts}.h5")

    def Save(self, output_file=None):
        """HDF5 file in the reference's layout: every edge's weight / bias / gradient_history datasets and step attributes,
        plus ``__lr_reduce_counter__`` and ``__current_iter__``; written to ``<name>temp`` and renamed (convnet.cc:666-684)."""
        from . import hdf5io
        if output_file is None:
            # ConvNet::Save() (src/convnet.cc:659-667): the checkpoint, then — with Polyak averaging on — the AVERAGED weights
            # beside it as <file>polyak, and the current weights restored
            fname = self.GetCheckpointFilename()
            self.Save(fname)
            if self.model_.polyak_after > 0:
                self.LoadPolyakWeights()
                self.Save(fname + "polyak")
                self.LoadCurrentWeights()
            return
        tmp = output_file + "temp"
        with hdf5io.File(tmp, "w") as f:
            for e in self.edges_:
                e.SaveParameters(f)
            f.WriteHDF5IntAttr("__lr_reduce_counter__", getattr(self, "lr_reduce_counter_", 0))
            f.WriteHDF5IntAttr("__current_iter__", self.current_iter_)
        os.replace(tmp, output_file)

    def Load(self, input_file=None):
        """Weights always; optimizer history + step only where the optimizer is allocated (a training net), so the same file
        serves resume and fprop-only use (edge_with_weight.cc:42-58).  Learning-rate reductions are re-applied."""
        from . import hdf5io
        with hdf5io.File(input_file or self.GetCheckpointFilename()) as f:
            for e in self.edges_:
                e.LoadParameters(f)
            self.lr_reduce_counter_ = f.ReadHDF5IntAttr("__lr_reduce_counter__", getattr(self, "lr_reduce_counter_", 0))
            for _ in range(self.lr_reduce_counter_):
                self.ReduceLearningRate(self.model_.reduce_lr_factor)
            self.current_iter_ = f.ReadHDF5IntAttr("__current_iter__", self.current_iter_)
