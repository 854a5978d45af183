"""Edges (operators) — mirror of src/edge.{h,cc}, edge_with_weight.cc, conv_edge.cc, fc_edge.cc,
maxpool_edge.cc, avgpool_edge.cc, response_norm_edge.cc, upsample_edge.cc, rgb_to_yuv_edge.cc: same class names, same
ComputeUp / ComputeDown / ComputeOuter / UpdateWeights contract, same parameter slicing.

DOWNSAMPLE is refused: the reference's class is dead (ChooseEdgeClass has the reason).
``fused`` selects the library's fused entry points (conv+bias+ReLU epilogue, one-pass bias
gradient); the unfused path issues exactly the reference's Matrix-call sequence.  What an edge class can
fuse it says itself (``CanFuseUp``, ``can_fuse_mask``); which of it a net uses is ConvNet's per-layer plan.
"""
import math
import os

import numpy as np

from ._lib import ConvDesc
from .matrix import Matrix
from .optimizer import Optimizer


def _divup(x, y):
    return (x + y - 1) // y


class Edge:
    can_fuse_mask = False   # ComputeDown(fuse_mask=post_scale) supported; the other classes are never handed one

    def CanFuseUp(self, dest):
        """Whether ComputeUp(fuse_relu=...) can apply layer ``dest``'s bias and activation in its epilogue."""
        return False

    @staticmethod
    def ChooseEdgeClass(edge_config):
        # src/edge.cc:19-66
        table = {"FC": FCEdge, "CONVOLUTIONAL": ConvEdge, "MAXPOOL": MaxPoolEdge, "AVERAGE_POOL": AvgPoolEdge,
                 "RESPONSE_NORM": ResponseNormEdge, "CONV_ONETOONE": ConvOneToOneEdge, "LOCAL": LocalEdge,
                 "UPSAMPLE": UpSampleEdge, "RGBTOYUV": RGBToYUVEdge}
        if edge_config.edge_type == "DOWNSAMPLE":
            # src/downsample_edge.cc:18-23 MULTIPLIES the image size by the factor where it must divide: the destination layer gets the
            # wrong size and the pool reads outside the image.  The edge is dead in the reference; there is nothing to mirror
            raise SystemExit(f"Error: Edge {edge_config.source}:{edge_config.dest}: edge_type DOWNSAMPLE is not supported: the reference "
                             "sizes its destination as image_size * sample_factor and reads outside the image.  Use AVERAGE_POOL with "
                             f"kernel_size = stride = sample_factor ({edge_config.sample_factor}): the same forward pass with a correct "
                             "backward pass.")
        if edge_config.edge_type not in table:
            raise SystemExit(f"Error: Undefined edge type {edge_config.edge_type} (out of hot-path scope).")
        return table[edge_config.edge_type](edge_config)

    @staticmethod
    def HasParameters(edge_config):
        return edge_config.edge_type in ("FC", "CONVOLUTIONAL", "LOCAL", "CONV_ONETOONE")

    @staticmethod
    def GetConvDesc(c):
        # src/edge.cc:83-106 — paddings are stored negated
        d = ConvDesc()
        d.num_input_channels = 0
        d.num_output_channels = 0
        d.kernel_size_y = c.kernel_size_y if c.has_kernel_size_y() else c.kernel_size
        d.kernel_size_x = c.kernel_size_x if c.has_kernel_size_x() else c.kernel_size
        d.kernel_size_t = c.kernel_size_t if c.has_kernel_size_t() else 1
        d.stride_y = c.stride_y if c.has_stride_y() else c.stride
        d.stride_x = c.stride_x if c.has_stride_x() else c.stride
        d.stride_t = c.stride_t
        d.padding_y = -(c.padding_y if c.has_padding_y() else c.padding)
        d.padding_x = -(c.padding_x if c.has_padding_x() else c.padding)
        d.padding_t = -c.padding_t
        d.num_groups = 1
        return d

    @staticmethod
    def GetNumModules(d, image_size_y, image_size_x, image_size_t):
        # src/edge.cc:108-114
        return ((image_size_y - 2 * d.padding_y - d.kernel_size_y) // d.stride_y + 1,
                (image_size_x - 2 * d.padding_x - d.kernel_size_x) // d.stride_x + 1,
                (image_size_t - 2 * d.padding_t - d.kernel_size_t) // d.stride_t + 1)

    def __init__(self, c):
        self.source_ = None
        self.dest_ = None
        self.source_node_ = c.source
        self.dest_node_ = c.dest
        self.source_node_slice_ = c.source_slice   # the slice of the source layer this edge reads, of the destination it writes;
        self.dest_node_slice_ = c.dest_slice       # "" = the whole layer (layer.py)
        self.tied_edge_name_ = c.tied_to
        self.tied_edge_ = None
        self.num_input_channels_ = 0
        self.num_output_channels_ = 0
        self.image_size_y_ = self.image_size_x_ = self.image_size_t_ = 1
        self.num_modules_y_ = self.num_modules_x_ = self.num_modules_t_ = 1
        self.mark_ = False
        self.block_backprop_ = c.block_backprop
        self.is_tied_ = bool(self.tied_edge_name_)
        self.grad_check_ = c.grad_check
        self.grad_check_num_params_ = c.grad_check_num_params
        self.grad_check_epsilon_ = list(c.grad_check_epsilon)
        # src/edge.cc:150-155: <source>[_<slice>]:<dest>[_<slice>]
        self.name_ = ":".join(n + ("_" + sl if sl else "") for n, sl in ((self.source_node_, self.source_node_slice_),
                                                                         (self.dest_node_, self.dest_node_slice_)))
        self.fused = False

    def GetDescription(self):
        return "Default edge."

    def SetTiedTo(self, e):
        self.tied_edge_ = e

    def SetInputChannels(self, a):
        self.num_input_channels_ = a

    def SetOutputChannels(self, a):
        self.num_output_channels_ = a
        Matrix.RegisterTempMemory(a, "Used for computing average length of incoming weight vectors.")

    def SetImageSize(self, y, x, t):
        self.image_size_y_, self.image_size_x_, self.image_size_t_ = y, x, t

    def _set_desc_channels(self, channel_end=True):
        """The channel fields of conv_desc_ (src/conv_edge.cc:52-58, maxpool_edge.cc:13-19).  LocalEdge::SetImageSize leaves the two
        *_channel_end fields as GetConvDesc made them (``channel_end=False``)."""
        d = self.conv_desc_
        d.num_input_channels = self.num_input_channels_
        d.num_output_channels = self.num_output_channels_
        if channel_end:
            d.input_channel_end = self.num_input_channels_
            d.output_channel_end = self.num_output_channels_
        return d

    def Initialize(self):
        pass

    def SetMemory(self, p):
        pass

    def SetGradMemory(self, p, hist=None, hist2=None):
        pass

    def GetParameterMemoryRequirement(self):
        return 0

    def ComputeOuter(self, input, deriv_output):
        pass

    def UpdateWeights(self):
        pass

    def SaveParameters(self, file):       # src/edge.cc: edges without parameters store nothing
        pass

    def LoadParameters(self, file, edge_name=None):
        pass

    def NotifyStart(self):
        pass

    def GetRMSWeight(self):
        return 0.0

    def SetSource(self, l):
        self.source_ = l

    def SetDest(self, l):
        self.dest_ = l

    def GetSource(self):
        return self.source_

    def GetDest(self):
        return self.dest_

    def GetSourceName(self):
        return self.source_node_

    def GetDestName(self):
        return self.dest_node_

    def GetSourceSliceName(self):
        return self.source_node_slice_

    def GetDestSliceName(self):
        return self.dest_node_slice_

    def GetName(self):
        return self.name_

    def SetMark(self):
        self.mark_ = True

    def HasMark(self):
        return self.mark_

    def HasNoParameters(self):
        return True

    def GetNumModulesY(self):
        return self.num_modules_y_

    def GetNumModulesX(self):
        return self.num_modules_x_

    def GetNumModulesT(self):
        return self.num_modules_t_

    def GetTiedEdgeName(self):
        return self.tied_edge_name_

    def IsTied(self):
        return self.is_tied_

    def IsBackPropBlocked(self):
        return self.block_backprop_

    def GradCheck(self):
        return self.grad_check_

    def GradCheckNumParams(self):
        return self.grad_check_num_params_

    def GradCheckEpsilon(self):
        return list(self.grad_check_epsilon_)


class EdgeWithWeight(Edge):
    """src/edge_with_weight.{h,cc}"""

    def __init__(self, c):
        super().__init__(c)
        self.weight_optimizer_ = Optimizer.ChooseOptimizer(c.weight_optimizer)
        self.bias_optimizer_ = None if c.has_no_bias else Optimizer.ChooseOptimizer(c.bias_optimizer)
        self.initialization_ = c.initialization
        self.init_wt_ = c.init_wt
        self.init_bias_ = c.init_bias
        self.pretrained_model_ = c.pretrained_model
        self.pretrained_edge_name_ = c.pretrained_edge_name      # empty: the edge's own "<source>:<dest>" (src/edge_with_weight.cc:17-19)
        self.has_no_bias_ = c.has_no_bias
        self.num_grads_received_ = 0
        self.num_shares_ = 1
        self.scale_gradients_ = c.scale_gradients
        self.weights_, self.grad_weights_, self.bias_, self.grad_bias_ = Matrix(), Matrix(), Matrix(), Matrix()
        self.history_slice_ = None   # optional flat optimizer-state slice handed in by ConvNet

    def HasNoParameters(self):
        return False

    def GetWeight(self):
        return self.weights_

    def GetGradWeight(self):
        return self.grad_weights_

    def GetBias(self):
        return self.bias_

    def GetGradBias(self):
        return self.grad_bias_

    # The matrices the passes work on: a tied edge uses (and accumulates into) those of the edge it is tied to
    # (src/edge_with_weight.cc:66-90).  No bias: None.
    def _owner(self):
        return self.tied_edge_ if self.is_tied_ else self

    def _w(self):
        return self._owner().weights_

    def _b(self):
        return None if self.has_no_bias_ else self._owner().bias_

    def _dw(self):
        return self._owner().grad_weights_

    def _db(self):
        return None if self.has_no_bias_ else self._owner().grad_bias_

    def SetTiedTo(self, e):
        if not isinstance(e, EdgeWithWeight):
            raise SystemExit(f"Error: Edge {self.GetName()} cannot be tied to edge {e.GetName()} which is not of the same type.")
        self.tied_edge_ = e
        e.num_shares_ += 1

    def GetNumGradsReceived(self):
        return self.tied_edge_.GetNumGradsReceived() if self.is_tied_ else self.num_grads_received_

    def IncrementNumGradsReceived(self):
        if self.is_tied_:
            self.tied_edge_.IncrementNumGradsReceived()
        else:
            self.num_grads_received_ += 1

    def ReduceLearningRate(self, factor):
        self.weight_optimizer_.ReduceLearningRate(factor)
        if self.bias_optimizer_:
            self.bias_optimizer_.ReduceLearningRate(factor)

    def _checkpoint_prefix(self):
        """The prefix of this edge's datasets in a checkpoint.  The reference's is <source>:<dest> (src/edge_with_weight.cc:27-64),
        kept for every edge on whole layers: their files stay the reference's.  It does not tell the groups of a grouped convolution
        apart (two edges between the same two layers), so an edge that names a slice uses its name, <source>[_<slice>]:<dest>[_<slice>]
        — the reference cannot write a checkpoint of such a net, so there is no file of its to stay compatible with."""
        if self.source_node_slice_ or self.dest_node_slice_:
            return self.name_
        return f"{self.source_node_}:{self.dest_node_}"

    def SaveParameters(self, file):
        # src/edge_with_weight.cc:27-40: "<prefix>:weight" / ":bias" + the optimizers' state under the same names
        if self.is_tied_:
            return
        name = f"{self._checkpoint_prefix()}:weight"
        self.weights_.WriteHDF5(file, name)
        self.weight_optimizer_.SaveParameters(file, name)
        if not self.has_no_bias_:
            name = f"{self._checkpoint_prefix()}:bias"
            self.bias_.WriteHDF5(file, name)
            self.bias_optimizer_.SaveParameters(file, name)

    def LoadParameters(self, file, edge_name=None):
        # src/edge_with_weight.cc:42-64 (optimizer state only if the optimizer has been allocated, i.e. when training)
        if self.is_tied_:
            return
        edge_name = edge_name or self._checkpoint_prefix()
        self.weights_.ReadHDF5(file, f"{edge_name}:weight")
        if self.weight_optimizer_.IsAllocated():
            self.weight_optimizer_.LoadParameters(file, f"{edge_name}:weight")
        if not self.has_no_bias_:
            self.bias_.ReadHDF5(file, f"{edge_name}:bias")
            if self.bias_optimizer_.IsAllocated():
                self.bias_optimizer_.LoadParameters(file, f"{edge_name}:bias")

    def UpdateWeights(self, batch=None):
        # src/edge_with_weight.cc:96-106.  `batch`: a list that collects the plain fused SGD steps of a whole net for ONE launch
        # (ConvNet.UpdateWeights -> optimizer.RunFusedSteps, one multi launch per optimizer kind); steps that are not plain run here as before.
        if self.is_tied_:
            return
        if self.num_grads_received_ < self.num_shares_:
            raise SystemExit("Error: Update called when all gradients were not received.")
        self.num_grads_received_ = 0
        pairs = [(self.weight_optimizer_, self.grad_weights_, self.weights_)]
        if not self.has_no_bias_:
            pairs.append((self.bias_optimizer_, self.grad_bias_, self.bias_))
        for opt, grad, param in pairs:
            item = opt.PlanFusedStep(grad, param) if batch is not None and hasattr(opt, "PlanFusedStep") else None
            if item is not None:
                batch.append(item)
            else:
                opt.Optimize(grad, param)

    def NotifyStart(self):
        self.weight_optimizer_.NotifyStart(self.weights_)
        if not self.has_no_bias_:
            self.bias_optimizer_.NotifyStart(self.bias_)

    def Initialize(self):
        # src/edge_with_weight.cc:108-143
        if self.is_tied_:
            return
        init = self.initialization_
        if init in ("DENSE_GAUSSIAN_SQRT_FAN_IN", "DENSE_GAUSSIAN"):
            self.weights_.FillWithRandn()
            init_wt = self.init_wt_
            if init == "DENSE_GAUSSIAN_SQRT_FAN_IN":
                init_wt /= math.sqrt(self.weights_.GetCols())
            self.weights_.Mult(init_wt)
        elif init in ("DENSE_UNIFORM_SQRT_FAN_IN", "DENSE_UNIFORM"):
            self.weights_.FillWithRand()
            self.weights_.Add(-0.5)
            init_wt = 2 * self.init_wt_
            if init == "DENSE_UNIFORM_SQRT_FAN_IN":
                init_wt /= math.sqrt(self.weights_.GetCols() / 3.0)
            self.weights_.Mult(init_wt)
        elif init == "CONSTANT":
            self.weights_.Set(self.init_wt_)
        elif init == "PRETRAINED":
            self._load_pretrained()
        else:
            raise SystemExit(f"Unknown / out-of-scope weight initialization type {init}.")
        if init != "PRETRAINED" and not self.has_no_bias_:       # a loaded bias stays (:140-142)
            self.bias_.Set(self.init_bias_)

    def _load_pretrained(self):
        """``initialization: PRETRAINED`` (src/edge_with_weight.cc:132-135): weight and bias come from ``pretrained_model``, stored there
        under ``pretrained_edge_name`` or this edge's own "<source>:<dest>" (the name ``SaveParameters`` stores it under)."""
        from . import hdf5io
        edge_name = self.pretrained_edge_name_ or self._checkpoint_prefix()
        try:
            file = hdf5io.File(self.pretrained_model_)
        except OSError as e:
            raise SystemExit(f"Edge {self.GetName()}: initialization PRETRAINED: {e}")
        with file:
            for what in ("weight",) if self.has_no_bias_ else ("weight", "bias"):
                if not file.Has(f"{edge_name}:{what}"):
                    raise SystemExit(f"Edge {self.GetName()}: initialization PRETRAINED: no dataset {edge_name}:{what} in {self.pretrained_model_}")
            self.LoadParameters(file, edge_name)

    def GetRMSWeight(self):
        temp = Matrix()
        num_hid = self.weights_.GetRows()
        Matrix.GetTemp(num_hid, 1, temp)
        self.weights_.SqSumAxis(temp, 1, 1, 0)
        temp.Sqrt()
        return temp.Sum() / num_hid

    # ---- parameter slicing: src/conv_edge.cc:72-136, local_edge.cc, fc_edge.cc.  An edge's slice of the flat parameter (and gradient)
    # buffer is a (rows, _input_size() + bias_cols) matrix: the weights first, then the bias, read as one row.  A subclass gives
    # _input_size() and _param_layout() = (rows, bias_cols, the weights' Shape4D or None).
    def _num_modules(self):
        return self.num_modules_y_ * self.num_modules_x_ * self.num_modules_t_

    def GetParameterMemoryRequirement(self):
        if self.is_tied_:
            return 0
        rows, bias_cols, _ = self._param_layout()
        return rows * (self._input_size() + (0 if self.has_no_bias_ else bias_cols))

    def _slice_params(self, p, w, b):
        rows, bias_cols, shape4d = self._param_layout()
        input_size = self._input_size()
        p.Reshape(rows, -1)
        p.GetSlice(w, 0, input_size)
        if shape4d is not None:
            w.SetShape4D(*shape4d)
        if not self.has_no_bias_:
            p.GetSlice(b, input_size, input_size + bias_cols)
            b.Reshape(1, -1)

    def SetMemory(self, p):
        if self.is_tied_:
            return
        self._slice_params(p, self.weights_, self.bias_)

    def SetGradMemory(self, p, hist=None, hist2=None):
        if self.is_tied_:
            return
        self._slice_params(p, self.grad_weights_, self.grad_bias_)
        rows, bias_cols, _ = self._param_layout()
        self._alloc_optimizers(rows, self._input_size(), bias_cols, hist, hist2)

    # ---- the bias after the up-GEMM and its gradient after the outer-GEMM.  ``shared`` = F: a conv edge's shared bias, one value per
    # filter, on the (N*My*Mx, F) view of a frame.  ``frames`` = None: one frame, used whole (src/conv_edge.cc:145-149, 210-221);
    # Mt: a 3-D edge, frame by frame through column slices of the (N*My*Mx, F*Mt) view (:153-168, 223-242).
    def _add_bias(self, output, shared=0, frames=None):
        b = self._b()
        if b is None:
            return
        if not shared:
            output.AddRowVec(b)
            return
        cols = output.GetCols()
        output.Reshape(-1, shared * (frames or 1))
        if frames is None:
            output.AddRowVec(b)
        else:
            for m in range(frames):
                output_slice = Matrix()
                output.GetSlice(output_slice, m * shared, (m + 1) * shared)
                output_slice.AddRowVec(b)
        output.Reshape(-1, cols)

    def _bias_grad(self, deriv_output, scale_targets, scale_outputs, shared=0, frames=None):
        db = self._db()
        if db is None:
            return
        if not shared:
            deriv_output.SumRows(db, scale_targets, scale_outputs)
            return
        db_temp = Matrix()
        Matrix.GetTemp(1, deriv_output.GetCols(), db_temp)
        deriv_output.SumRows(db_temp, 0, 1)
        db_temp.Reshape(-1, shared * (frames or 1))
        if frames is None:
            db_temp.SumRows(db, scale_targets, scale_outputs)
        else:
            for m in range(frames):   # (db.Mult(scale_targets) folded into the first frame's SumRows)
                db_temp_slice = Matrix()
                db_temp.GetSlice(db_temp_slice, m * shared, (m + 1) * shared)
                db_temp_slice.SumRows(db, scale_targets if m == 0 else 1, scale_outputs)

    def _alloc_optimizers(self, rows, cols, bias_cols, hist, hist2=None):
        """Optimizer state: either separate matrices (reference) or slices of a flat history
        buffer laid out exactly like the parameter slice (``hist``; ``hist2``: the same for the
        second-moment history, sliced for the optimizers that keep one)."""
        for h in (hist, hist2):
            if h is not None:
                h.Reshape(rows, -1)

        def part(h, opt, start, end):
            if h is None or (h is hist2 and not opt.NeedsSecondHistory()):
                return None
            m = Matrix()
            h.GetSlice(m, start, end)
            return m
        w_opt, b_opt = self.weight_optimizer_, self.bias_optimizer_
        w_opt.AllocateMemory(rows, cols, part(hist, w_opt, 0, cols), part(hist2, w_opt, 0, cols))
        if not self.has_no_bias_:
            b_opt.AllocateMemory(1, rows * bias_cols, part(hist, b_opt, cols, cols + bias_cols), part(hist2, b_opt, cols, cols + bias_cols))


class ConvEdge(EdgeWithWeight):
    """src/conv_edge.{h,cc}.  A source layer with image_size_t > 1 frames makes the edge a spatio-temporal (3-D) convolution
    (kernel_size_t, stride_t; time is the outermost index of activations and bank, include/convnet_hip.h): it then issues the reference's
    Conv3D* calls, the shared bias is added per output frame and its gradient summed over the frames (conv_edge.cc:153-168, 223-242)."""
    can_fuse_mask = True

    def __init__(self, c):
        super().__init__(c)
        self.conv_desc_ = Edge.GetConvDesc(c)
        self.shared_bias_ = c.shared_bias

    def GetConvDesc(self):
        return self.conv_desc_

    def SetImageSize(self, y, x, t):
        super().SetImageSize(y, x, t)
        d = self._set_desc_channels()
        self.num_modules_y_, self.num_modules_x_, self.num_modules_t_ = Edge.GetNumModules(d, y, x, t)
        if t != 1:
            if d.padding_t != 0:
                # the reference's 3-D loops assert padding_t == 0 (cudamat_conv3d_gemm.cu:23)
                raise SystemExit(f"Error: Edge {self.name_}: padding_t is not supported on a convolutional edge")
            if self.num_modules_t_ < 1:
                raise SystemExit(f"Error: Edge {self.name_}: kernel_size_t {d.kernel_size_t} exceeds the {t} frames of its source layer")

    def GetDescription(self):
        # src/conv_edge.cc:41-50 and Edge::GetDescription(conv_desc), src/edge.cc:116-123
        d = self.conv_desc_
        kt = f"-{d.kernel_size_t}" if d.kernel_size_t != 1 else ""
        it = f"-{self.image_size_t_}" if self.image_size_t_ != 1 else ""
        mt = f"-{self.num_modules_t_}" if self.num_modules_t_ != 1 else ""
        return (f"{self.name_} Convolutional Kernel: {d.kernel_size_y}-{d.kernel_size_x}-{d.num_input_channels}{kt} : "
                f"{d.num_output_channels} Layer: {self.image_size_y_}-{self.image_size_x_}{it} : {self.num_modules_y_}-{self.num_modules_x_}{mt}")

    def _input_size(self):
        d = self.conv_desc_
        return d.kernel_size_y * d.kernel_size_x * d.kernel_size_t * d.num_input_channels

    def _param_layout(self):
        # src/conv_edge.cc:72-108: one bias per filter (shared) or per filter and location
        d = self.conv_desc_
        return (d.num_output_channels, 1 if self.shared_bias_ else self._num_modules(),
                (d.num_output_channels, d.kernel_size_x, d.kernel_size_y, d.num_input_channels * d.kernel_size_t))

    def SetGradMemory(self, p, hist=None, hist2=None):
        # src/conv_edge.cc:110-136: the two-step shared-bias gradient takes a temp row (host bookkeeping, no library call)
        if not self.is_tied_ and self.shared_bias_ and not self.has_no_bias_:
            Matrix.RegisterTempMemory(self.conv_desc_.num_output_channels * self._num_modules(), "shared bias")
        super().SetGradMemory(p, hist, hist2)

    def CanFuseUp(self, dest):
        return self.has_no_bias_ or self.shared_bias_   # (the epilogue's bias is one value per filter)

    def _bias_view(self):
        """(shared, frames) of _add_bias / _bias_grad for this edge."""
        return (self.conv_desc_.num_output_channels if self.shared_bias_ else 0, self.num_modules_t_ if self.image_size_t_ != 1 else None)

    def ComputeUp(self, input, output, overwrite, train=True, fuse_relu=None):
        """src/conv_edge.cc:138-170.  ``fuse_relu`` (None = unfused reference sequence; True/False =
        fused conv+bias[+ReLU] epilogue; the caller then skips the layer's ApplyActivation)."""
        scale_targets = 0 if overwrite else 1
        three_d = self.image_size_t_ != 1
        if fuse_relu is not None and (self.has_no_bias_ or self.shared_bias_):
            (Matrix.Conv3DUpBiasAct if three_d else Matrix.ConvUpBiasAct)(input, self._w(), self._b(), output, self.conv_desc_,
                                                                          scale_targets, fuse_relu)
            return
        (Matrix.Conv3DUp if three_d else Matrix.ConvUp)(input, self._w(), output, self.conv_desc_, scale_targets)
        self._add_bias(output, *self._bias_view())

    def ComputeDown(self, deriv_output, input, output, deriv_input, overwrite, fuse_mask=None):
        """src/conv_edge.cc:172-181.  ``fuse_mask=post_scale`` additionally applies the source layer's
        ReLU' (mask = its state, ``input``) and dropout' scale in the kernel epilogue."""
        three_d = self.image_size_t_ != 1
        if fuse_mask is not None:
            (Matrix.Conv3DDownMask if three_d else Matrix.ConvDownMask)(deriv_output, self._w(), input, deriv_input, self.conv_desc_,
                                                                        0 if overwrite else 1, fuse_mask)
            return
        (Matrix.Conv3DDown if three_d else Matrix.ConvDown)(deriv_output, self._w(), deriv_input, self.conv_desc_, 0 if overwrite else 1)

    def ComputeOuter(self, input, deriv_output):
        # src/conv_edge.cc:183-245 (GEMM build: partial sums forced to one chunk, :11-17)
        dw = self._dw()
        scale_targets = 1 if self.GetNumGradsReceived() > 0 else 0
        scale_outputs = self.scale_gradients_ / input.GetRows()
        d = self.conv_desc_
        three_d = self.image_size_t_ != 1
        if self.fused and self.shared_bias_ and not self.has_no_bias_:
            (Matrix.Conv3DOutpBias if three_d else Matrix.ConvOutpBias)(input, deriv_output, dw, self._db(), d, scale_targets, scale_outputs)
        else:
            if three_d:
                Matrix.Conv3DOutp(input, deriv_output, dw, d, scale_targets, scale_outputs)
            else:
                Matrix.ConvOutp(input, deriv_output, dw, d, self.num_modules_y_, self.num_modules_x_, scale_targets, scale_outputs)
            self._bias_grad(deriv_output, scale_targets, scale_outputs, *self._bias_view())
        self.IncrementNumGradsReceived()


class LocalEdge(EdgeWithWeight):
    """src/local_edge.{h,cc}: a locally connected layer — a convolution whose every module (output pixel) has its own filter bank.

    Parameter slice (F, input_size + bias_locs), exactly as LocalEdge::SetMemory lays it out:
    * weights: the first input_size = Kx*Ky*C*My*Mx columns, Shape4D (F, Kx, Ky, C*My*Mx); module m = my*Mx + mx owns the F*K floats
      at m*F*K (K = Kx*Ky*C), element (f, c, ky, kx) of a block at f + F*(kx + Kx*(ky + Ky*c)) — a conv bank per module;
    * bias: the next bias_locs = My*Mx columns, i.e. an (F, M) block, read as (1, F*M): ComputeUp adds element j to output column j
      (AddRowVec), ComputeOuter sums deriv_output over the images into it.  There is no shared bias for local edges.
    ComputeUp / ComputeDown / ComputeOuter issue the reference's Matrix calls (LocalUp / LocalDown / LocalOutp, src/matrix.cc:859-893);
    ``fuse_relu`` selects localUpBiasAct (bias and ReLU in the kernel's epilogue)."""

    def __init__(self, c):
        super().__init__(c)
        self.conv_desc_ = Edge.GetConvDesc(c)

    def GetConvDesc(self):
        return self.conv_desc_

    def SetTiedTo(self, e):
        super().SetTiedTo(e)
        if not isinstance(e, LocalEdge):
            raise SystemExit(f"Error: Edge {self.GetName()} cannot be tied to edge {e.GetName()} which is not of the same type.")
        self.conv_desc_ = e.GetConvDesc().copy()

    def SetImageSize(self, y, x, t):
        super().SetImageSize(y, x, t)
        d = self._set_desc_channels(channel_end=False)
        self.num_modules_y_, self.num_modules_x_, self.num_modules_t_ = Edge.GetNumModules(d, y, x, t)
        if t != 1:
            raise SystemExit("3-D locally connected layers are out of hot-path scope")

    def GetDescription(self):
        # src/local_edge.cc:GetDescription (Edge::GetDescription(conv_desc): kernel y-x-input channels : output channels)
        d = self.conv_desc_
        return (f"{self.name_}  Local Kernel: {d.kernel_size_y}-{d.kernel_size_x}-{d.num_input_channels} : {d.num_output_channels}"
                f" Layer: {self.image_size_y_}-{self.image_size_x_} : {self.num_modules_y_}-{self.num_modules_x_}")

    def _input_size(self):
        d = self.conv_desc_
        return d.kernel_size_x * d.kernel_size_y * d.kernel_size_t * d.num_input_channels * self._num_modules()

    def _param_layout(self):
        d = self.conv_desc_
        return (d.num_output_channels, self._num_modules(),
                (d.num_output_channels, d.kernel_size_x, d.kernel_size_y, d.num_input_channels * self.num_modules_y_ * self.num_modules_x_))

    def CanFuseUp(self, dest):
        return True   # localUpBiasAct: the (per-column) bias and the ReLU in the kernel's epilogue

    def ComputeUp(self, input, output, overwrite, train=True, fuse_relu=None):
        scale_targets = 0 if overwrite else 1
        if fuse_relu is not None:
            Matrix.LocalUpBiasAct(input, self._w(), self._b(), output, self.conv_desc_, scale_targets, fuse_relu)
            return
        Matrix.LocalUp(input, self._w(), output, self.conv_desc_, scale_targets)
        self._add_bias(output)

    def ComputeDown(self, deriv_output, input, output, deriv_input, overwrite, fuse_mask=None):
        assert fuse_mask is None
        Matrix.LocalDown(deriv_output, self._w(), deriv_input, self.conv_desc_, 0 if overwrite else 1)

    def ComputeOuter(self, input, deriv_output):
        scale_targets = 1 if self.GetNumGradsReceived() > 0 else 0
        scale_outputs = self.scale_gradients_ / input.GetRows()
        Matrix.LocalOutp(input, deriv_output, self._dw(), self.conv_desc_, scale_targets, scale_outputs)
        self._bias_grad(deriv_output, scale_targets, scale_outputs)
        self.IncrementNumGradsReceived()


class FCEdge(EdgeWithWeight):
    """src/fc_edge.{h,cc}"""
    can_fuse_mask = True

    def _input_size(self):
        return self.image_size_y_ * self.image_size_x_ * self.image_size_t_ * self.num_input_channels_

    def _param_layout(self):
        return self.num_output_channels_, 1, None

    def GetDescription(self):
        return f"{self.name_} Fully Connected :{self.image_size_y_}-{self.image_size_x_}-{self.num_input_channels_}:{self.num_output_channels_}"

    def CanFuseUp(self, dest):
        return True

    def ComputeUp(self, input, output, overwrite, train=True, fuse_relu=None):
        # src/fc_edge.cc:51-61
        scale_targets = 0 if overwrite else 1
        if fuse_relu is not None:
            Matrix.DotBiasAct(input, self._w(), self._b(), output, scale_targets, 1, False, True, fuse_relu)
            return
        Matrix.Dot(input, self._w(), output, scale_targets, 1, False, True)
        self._add_bias(output)

    def ComputeDown(self, deriv_output, input, output, deriv_input, overwrite, fuse_mask=None):
        # src/fc_edge.cc:63-68
        if fuse_mask is not None:
            Matrix.DotMask(deriv_output, self._w(), input, deriv_input, 0 if overwrite else 1, 1, fuse_mask)
            return
        Matrix.Dot(deriv_output, self._w(), deriv_input, 0 if overwrite else 1, 1)

    def ComputeOuter(self, input, deriv_output, batch_size=None):
        # src/fc_edge.cc:70-81.  ``batch_size``: the layer's batch where ``input`` is a view with other rows (ConvOneToOneEdge)
        scale_targets = 1 if self.GetNumGradsReceived() > 0 else 0
        if batch_size is None:
            batch_size = input.GetRows()
        scale_outputs = self.scale_gradients_ / batch_size
        Matrix.Dot(deriv_output, input, self._dw(), scale_targets, scale_outputs, True, False)
        self._bias_grad(deriv_output, scale_targets, scale_outputs)
        self.IncrementNumGradsReceived()


class ConvOneToOneEdge(FCEdge):
    """src/conv_onetoone_edge.{h,cc}: a 1x1 convolution (network-in-network layer) = the FC GEMMs on the
    (N*X*Y, C) view of the same CHWN bytes, so pixel and image together form the contiguous "image" axis of the
    gather-GEMM kernels.  Everything but the reshapes is FCEdge's."""

    def SetImageSize(self, y, x, t):
        # src/conv_onetoone_edge.cc:8-13
        Edge.SetImageSize(self, y, x, t)
        self.num_modules_y_, self.num_modules_x_, self.num_modules_t_ = y, x, t
        if t != 1:
            # the (N*X*Y, C) view groups by channel only for one frame: with time outermost a column would mix channels and frames
            raise SystemExit(f"Error: Edge {self.name_}: CONV_ONETOONE is not supported on a layer with image_size_t > 1 ({t} frames)")

    def _input_size(self):
        return self.num_input_channels_

    def GetDescription(self):
        return (f"{self.name_}  One-to-One Convolutional Kernel: {self.num_input_channels_} : {self.num_output_channels_} Layer: "
                f"{self.image_size_y_}-{self.image_size_x_}-{self.num_input_channels_} : {self.num_modules_y_}-{self.num_modules_x_}-"
                f"{self.num_output_channels_}")

    class _Flat:
        """with-block: view activations as (N*X*Y, channels) and restore (batch, -1) on exit (:58-59,72-73)."""

        def __init__(self, *pairs):
            self.pairs = [(m, ch) for m, ch in pairs if m is not None]

        def __enter__(self):
            self.rows = [m.GetRows() for m, _ in self.pairs]
            for m, ch in self.pairs:
                m.Reshape(-1, ch)

        def __exit__(self, *exc):
            for (m, _), rows in zip(self.pairs, self.rows):
                m.Reshape(rows, -1)

    def ComputeUp(self, input, output, overwrite, train=True, fuse_relu=None):
        with self._Flat((input, self.num_input_channels_), (output, self.num_output_channels_)):
            FCEdge.ComputeUp(self, input, output, overwrite, train, fuse_relu)

    def ComputeDown(self, deriv_output, input, output, deriv_input, overwrite, fuse_mask=None):
        with self._Flat((deriv_output, self.num_output_channels_), (deriv_input, self.num_input_channels_),
                        (input if fuse_mask is not None else None, self.num_input_channels_)):
            FCEdge.ComputeDown(self, deriv_output, input, output, deriv_input, overwrite, fuse_mask)

    def ComputeOuter(self, input, deriv_output):
        # scale_gradients / batch_size uses the layer's batch (rows before the reshape), :92-104
        batch_size = input.GetRows()
        with self._Flat((input, self.num_input_channels_), (deriv_output, self.num_output_channels_)):
            FCEdge.ComputeOuter(self, input, deriv_output, batch_size)


class _PoolEdge(Edge):
    def __init__(self, c):
        super().__init__(c)
        self.conv_desc_ = Edge.GetConvDesc(c)

    def GetConvDesc(self):
        return self.conv_desc_

    def SetImageSize(self, y, x, t):
        # src/maxpool_edge.cc:13-25
        super().SetImageSize(y, x, t)
        d = self._set_desc_channels()
        if d.kernel_size_y <= 0:
            d.kernel_size_y = y
        if d.kernel_size_x <= 0:
            d.kernel_size_x = x
        if d.kernel_size_t <= 0:
            d.kernel_size_t = t
        self.num_modules_y_, self.num_modules_x_, self.num_modules_t_ = Edge.GetNumModules(d, y, x, t)
        if self.num_modules_t_ < 1:
            raise SystemExit(f"Error: Edge {self.name_}: kernel_size_t {d.kernel_size_t} exceeds the {t} frames of its source layer")

    def HasTimeWindow(self):
        """The windows are Ky x Kx x Kt boxes over the frames of a clip (include/convnet_hip.h: pooling over time)."""
        d = self.conv_desc_
        return self.image_size_t_ > 1 and (d.kernel_size_t > 1 or d.stride_t > 1 or d.padding_t != 0)


_POOL_MASK = os.environ.get("CONVNET_POOL_MASK", "1") != "0"   # A/B switch (tools/profile_round.sh): 0 = the reference's call pair on the fused path too


class MaxPoolEdge(_PoolEdge):
    """src/maxpool_edge.{h,cc}.  With the host's fused entry points on (ConvNet(fused=True) sets ``fused``) the forward pass also records
    the window masks (include/convnet_hip.h: MaxPoolMask) and the backward pass routes the derivatives from them alone — it reads neither
    the layer's input (1.19 GB for AlexNet's pool1) nor its maxima.
    The reference's MaxPoolUndo routes a derivative to the inputs that equal the pool layer's state AS BACKPROP SEES IT, i.e. after the
    layer's activation and dropout (src/convnet.cc:377-405, src/maxpool_edge.cc:60-65); the mask records the raw window maximum.  The two
    agree only when the destination layer has no dropout and a linear or ReLU activation (ReLU' zeroes the derivative wherever ReLU moved
    the maximum), so ConvNet sets ``mask_legal_`` from the destination and only then is the mask pair used; it is bit-identical to the
    reference's call pair there.  Other destinations, geometries without a mask kernel, and a ComputeDown that is handed other matrices
    than the ComputeUp before it take the reference's calls."""
    can_fuse_mask = True

    def __init__(self, c):
        super().__init__(c)
        self.mask_legal_ = False   # set by ConvNet's per-layer plan from the destination layer (see the class docstring)
        self.mask_ = None
        self.mask_for_ = None   # (input data pointer, output data pointer, batch) of the ComputeUp that wrote mask_
        self.mask_refused_ = set()   # (batch, input size, output size) the mask kernel refused: no mask, no call from then on

    def MaskEligible(self):
        # (the mask kernels are 2-D: a window with a time extent takes the reference's call pair)
        return self.fused and self.mask_legal_ and _POOL_MASK and not self.HasTimeWindow()

    def ComputeUp(self, input, output, overwrite, train=True, fuse_relu=None):
        if not overwrite:
            raise SystemExit(" In MaxPoolEdge::ComputeUp() : some other layer is writing to this maxpool layer's output as well. Not implemented.")
        self.mask_for_ = None
        key = (output.GetRows(), input.GetCols(), output.GetCols())
        if train and self.MaskEligible() and key not in self.mask_refused_:
            need = (output.GetRows(), (output.GetCols() + 1) // 2)
            if self.mask_ is None or (self.mask_.GetRows(), self.mask_.GetCols()) != need:
                self.mask_ = Matrix()
                self.mask_.AllocateGPUMemory(need[0], need[1], "maxpool mask")
            if Matrix.ConvMaxPoolMask(input, output, self.mask_, self.conv_desc_):
                self.mask_for_ = (input.mat_.data_device, output.mat_.data_device, output.GetRows())
                return
            # refused by geometry and batch.  The 16-byte alignment it also checks holds for whole layer buffers, and for the slices
            # of a layer whenever the batch is a multiple of 4 (a slice starts batch * pixels * channels floats in) — which the
            # kernel asks for anyway; the key holds for this edge's own matrices, which never change
            self.mask_refused_.add(key)
            self.mask_ = None
        Matrix.ConvMaxPool(input, output, self.conv_desc_)

    def ComputeDown(self, deriv_output, input, output, deriv_input, overwrite, fuse_mask=None):
        relu = fuse_mask is not None and fuse_mask == 1.0
        if self.mask_for_ is not None and self.mask_for_ == (input.mat_.data_device, output.mat_.data_device, output.GetRows()) and (overwrite or not relu):
            Matrix.ConvMaxPoolUndoMask(deriv_output, self.mask_, deriv_input, self.conv_desc_, 0 if overwrite else 1, relu)
            return
        if relu:
            Matrix.ConvMaxPoolUndoRelu(input, deriv_output, output, deriv_input, self.conv_desc_, 0 if overwrite else 1)
            return
        Matrix.ConvMaxPoolUndo(input, deriv_output, output, deriv_input, self.conv_desc_, 0 if overwrite else 1)


class AvgPoolEdge(_PoolEdge):
    """src/avgpool_edge.{h,cc}"""

    def ComputeUp(self, input, output, overwrite, train=True, fuse_relu=None):
        if not overwrite:
            raise SystemExit(" In AvgPoolEdge::ComputeUp() : some other layer is writing to this layer's output as well. Not implemented.")
        Matrix.ConvAvgPool(input, output, self.conv_desc_)

    def ComputeDown(self, deriv_output, input, output, deriv_input, overwrite, fuse_mask=None):
        assert fuse_mask is None
        Matrix.ConvAvgPoolUndo(deriv_output, deriv_input, self.conv_desc_, 0 if overwrite else 1)


class ResponseNormEdge(Edge):
    """src/response_norm_edge.{h,cc}"""

    def __init__(self, c):
        super().__init__(c)
        self.num_filters_response_norm_ = 0
        self.blocked_ = c.response_norm_in_blocks
        self.add_scale_ = c.add_scale
        self.pow_scale_ = c.pow_scale
        self.frac_of_filters_response_norm_ = c.frac_of_filters_response_norm

    def SetImageSize(self, y, x, t):
        super().SetImageSize(y, x, t)
        self.num_modules_y_, self.num_modules_x_, self.num_modules_t_ = y, x, t
        # (int) truncation of a *float* product, as in C++ (src/response_norm_edge.cc:37-38)
        self.num_filters_response_norm_ = int(np.float32(self.frac_of_filters_response_norm_) * np.float32(self.num_input_channels_))

    def CanFuseUp(self, dest):
        return dest.is_relu   # the ReLU of an rnorm-fed layer rides in the rnorm kernel; other activations do not

    def ComputeUp(self, input, output, overwrite, train=True, fuse_relu=None):
        # fuse_relu=True: the destination layer's ReLU (layer.cc:549) is applied by the same kernel
        if self.image_size_t_ > 1:   # src/response_norm_edge.cc:46-50: frame by frame
            Matrix.ConvResponseNormCrossMap3D(input, output, self.num_input_channels_, self.num_filters_response_norm_,
                                              self.add_scale_, self.pow_scale_, self.blocked_, self.image_size_t_, relu=bool(fuse_relu))
            return
        Matrix.ConvResponseNormCrossMap(input, output, self.num_input_channels_, self.num_filters_response_norm_,
                                        self.add_scale_, self.pow_scale_, self.blocked_, relu=bool(fuse_relu))

    def ComputeDown(self, deriv_output, input, output, deriv_input, overwrite, fuse_mask=None):
        assert fuse_mask is None
        if self.image_size_t_ > 1:
            Matrix.ConvResponseNormCrossMapUndo3D(deriv_output, input, output, deriv_input, self.num_input_channels_,
                                                  self.num_filters_response_norm_, self.add_scale_, self.pow_scale_, self.blocked_,
                                                  self.image_size_t_)
            return
        Matrix.ConvResponseNormCrossMapUndo(deriv_output, input, output, deriv_input, self.num_input_channels_,
                                            self.num_filters_response_norm_, self.add_scale_, self.pow_scale_, self.blocked_)


class UpSampleEdge(Edge):
    """src/upsample_edge.{h,cc}: every pixel of the source map is repeated sample_factor x sample_factor times (include/convnet_hip.h:
    UpSampleGemm).  With ``overwrite`` false the repeated map is ADDED to the destination, so an upsampled coarse map and a convolution
    can sum into one layer.
    ComputeDown is the reference's: the MEAN over each factor x factor block of derivatives, written over whatever ``deriv_input`` held —
    ``overwrite`` is ignored.  The adjoint of the replication would be the sum, so the gradients below this edge are 1 / factor^2 of the
    true ones (NOTES.md; the reference's own GradChecker says so), and a second back-propagated edge out of the same source layer would
    lose its derivative: ConvNet.BuildNet refuses that net."""

    def __init__(self, c):
        super().__init__(c)
        self.sample_factor_ = c.sample_factor
        if self.sample_factor_ < 1:
            raise SystemExit(f"Error: Edge {self.name_}: sample_factor {self.sample_factor_} is not supported on an UPSAMPLE edge: "
                             "it must be at least 1.")

    def SetImageSize(self, y, x, t):
        # src/upsample_edge.cc:18-23
        super().SetImageSize(y, x, t)
        if t > 1:
            raise SystemExit(f"Error: Edge {self.name_}: UPSAMPLE is not supported on a layer with image_size_t > 1 ({t} frames)")
        self.num_modules_y_, self.num_modules_x_, self.num_modules_t_ = y * self.sample_factor_, x * self.sample_factor_, t

    def GetDescription(self):
        # src/upsample_edge.cc:8-16 (two blanks behind the name and a trailing newline, as the reference writes them)
        return (f"{self.name_}  Upsample factor {self.sample_factor_} Layer: {self.image_size_y_}-{self.image_size_x_}-"
                f"{self.num_input_channels_} : {self.num_modules_y_}-{self.num_modules_x_}-{self.num_output_channels_}\n")

    def ComputeUp(self, input, output, overwrite, train=True, fuse_relu=None):
        Matrix.ConvUpSample(input, output, self.sample_factor_, 0 if overwrite else 1)

    def ComputeDown(self, deriv_output, input, output, deriv_input, overwrite, fuse_mask=None):
        assert fuse_mask is None
        Matrix.ConvDownSample(deriv_output, deriv_input, self.sample_factor_)


class RGBToYUVEdge(Edge):
    """src/rgb_to_yuv_edge.{h,cc}: the colour transform of include/convnet_hip.h (RGBToYUV) on a 3-channel source.  The reference class
    never sets num_modules, so its destination comes out 1 x 1; here the destination has the source's size.  No backward pass."""

    def SetImageSize(self, y, x, t):
        super().SetImageSize(y, x, t)
        if t > 1:
            raise SystemExit(f"Error: Edge {self.name_}: RGBTOYUV is not supported on a layer with image_size_t > 1 ({t} frames)")
        if self.num_input_channels_ != 3 or self.num_output_channels_ != 3:
            raise SystemExit(f"Error: Edge {self.name_}: RGBTOYUV needs 3 channels in and out: num_channels is {self.num_input_channels_} "
                             f"on its source and {self.num_output_channels_} on its destination.")
        self.num_modules_y_, self.num_modules_x_, self.num_modules_t_ = y, x, t

    def GetDescription(self):
        return f"{self.name_} RGB to YUV {self.image_size_y_}-{self.image_size_x_}"

    def ComputeUp(self, input, output, overwrite, train=True, fuse_relu=None):
        if not overwrite:
            raise SystemExit(f"Error: Edge {self.name_}: some other edge is writing to this RGBTOYUV edge's destination as well: "
                             "the transform overwrites it.")
        Matrix.ConvRGBToYUV(input, output)

    def ComputeDown(self, deriv_output, input, output, deriv_input, overwrite, fuse_mask=None):
        raise SystemExit("RGBtoYUV backprop Not implemented.")   # src/rgb_to_yuv_edge.cc:17-22
