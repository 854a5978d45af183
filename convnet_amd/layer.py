"""Layers — mirror of src/layer.{h,cc} for the hot path: Linear / ReLU / Logistic / Softmax / Softmax-distribution layers with
binary dropout, batch normalisation, their losses and metrics, and layer slices (``layer_slice``): named channel ranges of one layer
that edges read (``source_slice``) or write (``dest_slice``) on their own — grouped convolutions and channel concatenation.  In the
CHWN layout a channel range is a contiguous column range, so a slice is a get_slice view of the state and of the derivative with its
own Shape4D and its own add-or-overwrite flags; the slices lie in NAME order from column 0 (the reference keeps them in std::maps), a
non-zero ``num_channels`` of the layer itself sits behind the last slice.  Layer-level passes (activation, dropout, loss) stay on the
whole layer.  DESIGN.md §2.9 has the supported and the refused sets.  Gaussian dropout (``gaussian_dropout`` with ``dropprob`` as the
noise's standard deviation, ``max_act_gaussian_dropout``) runs on LINEAR, RECTIFIED_LINEAR and LOGISTIC hidden and
input layers: unfused as the reference's call sequence on a stored noise matrix — allocated for every such layer, which the reference
forgets for most classes — and fused as one pass forward and one backward that redraws the noise from the forward pass's RNG call id.
The model-parallel state copies are out of scope."""
import numpy as np

from .loss_functions import LossFunction
from .matrix import Matrix
from .optimizer import Optimizer


class Layer:
    @staticmethod
    def ChooseLayerClass(config):
        # src/layer.cc:8-32
        a = config.activation
        if a == "LINEAR":
            return LinearLayer(config)
        if a == "LOGISTIC":
            return LogisticLayer(config)
        if a == "RECTIFIED_LINEAR":
            return ReLULayer(config)
        if a == "SOFTMAX":
            return SoftmaxLayer(config)
        if a == "SOFTMAX_DIST":
            return SoftmaxDistLayer(config)
        raise SystemExit(f"Undefined layer type {a} (out of hot-path scope).")

    def __init__(self, config):
        self.name_ = config.name
        self.num_channels_ = config.num_channels
        self.is_input_ = True
        self.is_output_ = True
        self.dropprob_ = config.dropprob
        self.dropout_scale_up_at_train_time_ = True
        self.gaussian_dropout_ = config.gaussian_dropout
        self.image_size_y_ = config.image_size_y
        self.image_size_x_ = config.image_size_x
        self.image_size_t_ = config.image_size_t
        self.store_dropout_noise_ = self.dropprob_ > 0
        self.loss_ = None
        self.performance_ = None
        self.loss_function_ = config.loss_function
        self.performance_metric_ = config.performance_metric
        self.loss_function_weight_ = config.loss_function_weight
        self.has_tied_data_ = bool(config.tied_data)
        self.incoming_edge_ = []
        self.outgoing_edge_ = []
        self.state_ = Matrix()
        self.deriv_ = Matrix()
        self.data_ = Matrix()
        self.dropout_noise_ = Matrix()
        # Gaussian dropout (src/layer.cc:369-377, 399-404): dropprob is the noise's standard deviation.  What the layer's place in the
        # graph decides (no output layer, the layer class) is checked by ConvNet._check_gaussian_dropout
        self.max_act_gaussian_dropout_ = config.max_act_gaussian_dropout
        self.gaussian_call_id_ = None   # fused: the RNG call id of the last training forward pass, from which the backward pass redraws
        if self.gaussian_dropout_:
            if not np.isfinite(self.dropprob_):
                raise SystemExit(f"gaussian_dropout on layer {self.name_}: dropprob (the noise's standard deviation) is {self.dropprob_}, "
                                 "not a finite number")
            if not self.dropprob_ > 0:
                # (the reference silently does nothing)
                raise SystemExit(f"gaussian_dropout on layer {self.name_}: dropprob is {self.dropprob_}; it is the standard deviation of "
                                 "the noise and must be positive")
        elif self.max_act_gaussian_dropout_ > 0:
            # (ignored silently by the reference)
            raise SystemExit(f"max_act_gaussian_dropout on layer {self.name_} is set ({self.max_act_gaussian_dropout_}) without "
                             "gaussian_dropout: it clips the state after Gaussian noise only")
        # slices: src/layer.cc:66-73.  name -> channels in NAME order (std::map), which is also the order of their columns
        self.slice_channels_ = {}
        for s in config.layer_slice:
            self.slice_channels_[s.name] = s.num_channels
            self.num_channels_ += s.num_channels
        self.slice_channels_ = dict(sorted(self.slice_channels_.items()))
        self.state_slices_, self.deriv_slices_ = {}, {}
        self.add_or_overwrite_state_ = {n: True for n in ("", *self.slice_channels_)}
        self.add_or_overwrite_deriv_ = dict(self.add_or_overwrite_state_)
        # batch normalisation (src/layer.cc:60-64; the optimizer configs were merged with the model's defaults by ConvNet)
        self.batch_normalize_ = bool(config.batch_normalize)
        self.bn_f_ = config.bn_f
        self.bn_epsilon_ = config.bn_epsilon
        self.gamma_optimizer_ = self.beta_optimizer_ = None
        if self.batch_normalize_:
            self.gamma_optimizer_ = Optimizer.ChooseOptimizer(config.gamma_optimizer)
            self.beta_optimizer_ = Optimizer.ChooseOptimizer(config.beta_optimizer)
        self.gamma_, self.beta_, self.grad_gamma_, self.grad_beta_ = Matrix(), Matrix(), Matrix(), Matrix()
        self.mu_, self.sigma_, self.batch_mu_, self.batch_sigma_ = Matrix(), Matrix(), Matrix(), Matrix()
        self.fused = False

    # ---- graph ----------------------------------------------------------------------------------------
    def AddIncoming(self, e):
        self.is_input_ = False
        self.incoming_edge_.append(e)

    def AddOutgoing(self, e):
        self.is_output_ = False
        self.outgoing_edge_.append(e)

    def GetName(self):
        return self.name_

    def _no_slice(self, slice_):
        raise SystemExit(f"Layer {self.name_} does not contain a slice called {slice_}")

    def GetNumChannels(self, slice_=""):
        # src/layer.cc:334-348
        if not slice_:
            return self.num_channels_
        if slice_ not in self.slice_channels_:
            self._no_slice(slice_)
        return self.slice_channels_[slice_]

    def HasSlices(self):
        return bool(self.slice_channels_)

    def GetSliceChannelRange(self, slice_):
        """(first channel, one past the last) of a slice: name order from channel 0 (SetupSlices)."""
        if slice_ not in self.slice_channels_:
            self._no_slice(slice_)
        start = 0
        for n, c in self.slice_channels_.items():
            if n == slice_:
                return start, start + c
            start += c

    def IsInput(self):
        return self.is_input_

    def IsOutput(self):
        return self.is_output_

    def GetSizeY(self):
        return self.image_size_y_

    def GetSizeX(self):
        return self.image_size_x_

    def GetSizeT(self):
        return self.image_size_t_

    def SetSize(self, y, x, t):
        self.image_size_y_, self.image_size_x_, self.image_size_t_ = y, x, t

    def GetState(self, slice_=""):
        # src/layer.cc:294-305
        if not slice_:
            return self.state_
        if slice_ not in self.state_slices_:
            self._no_slice(slice_)
        return self.state_slices_[slice_]

    def GetDeriv(self, slice_=""):
        if not slice_:
            return self.deriv_
        if slice_ not in self.deriv_slices_:
            self._no_slice(slice_)
        return self.deriv_slices_[slice_]

    def GetData(self):
        return self.data_

    # add-or-overwrite bookkeeping: src/layer.cc:307-332.  One flag for the whole layer ("") and one per slice, independent of each other
    def AddOrOverwriteState(self, slice_=""):
        if slice_ not in self.add_or_overwrite_state_:
            self._no_slice(slice_)
        v = self.add_or_overwrite_state_[slice_]
        self.add_or_overwrite_state_[slice_] = False
        return v

    def AddOrOverwriteDeriv(self, slice_=""):
        if slice_ not in self.add_or_overwrite_deriv_:
            self._no_slice(slice_)
        v = self.add_or_overwrite_deriv_[slice_]
        self.add_or_overwrite_deriv_[slice_] = False
        return v

    def ResetAddOrOverwrite(self):
        for flags in (self.add_or_overwrite_state_, self.add_or_overwrite_deriv_):
            for n in flags:
                flags[n] = True

    def UseBatchNormalization(self):
        return self.batch_normalize_

    def NotifyStart(self):
        # src/layer.cc:520-525
        if self.batch_normalize_:
            self.gamma_optimizer_.NotifyStart(self.gamma_)
            self.beta_optimizer_.NotifyStart(self.beta_)

    # ---- memory: src/layer.cc:238-288 ----------------------------------------------------------------
    def SetupSlices(self):
        """src/layer.cc:238-250: slice s is the column range [start, start + pixels * channels_s) of the state and of the derivative."""
        num_pixels = self.image_size_y_ * self.image_size_x_ * self.image_size_t_
        batch_size = self.state_.GetRows()
        for n, c in self.slice_channels_.items():
            first, last = self.GetSliceChannelRange(n)
            for whole, views in ((self.state_, self.state_slices_), (self.deriv_, self.deriv_slices_)):
                v = views[n] = Matrix()
                whole.GetSlice(v, num_pixels * first, num_pixels * last)
                v.SetShape4D(batch_size, self.image_size_x_, self.image_size_y_, c * self.image_size_t_)

    def AllocateMemory(self, batch_size):
        num_pixels = self.image_size_y_ * self.image_size_x_ * self.image_size_t_
        self.state_.AllocateGPUMemory(batch_size, num_pixels * self.num_channels_, self.name_ + " state")
        self.deriv_.AllocateGPUMemory(batch_size, num_pixels * self.num_channels_, self.name_ + " deriv")
        for m in (self.state_, self.deriv_):
            m.SetShape4D(batch_size, self.image_size_x_, self.image_size_y_, self.num_channels_ * self.image_size_t_)
        if self.gaussian_dropout_:
            # The unfused sequence multiplies by a stored noise matrix and divides by it again, whatever the layer's class, input layers
            # included (the reference allocates none for the classes that clear the flag, and then runs on an empty matrix); the fused
            # entries draw the noise again from the call id and store nothing
            self.store_dropout_noise_ = not self.FusedGaussianDropout()
        elif self.is_input_:
            self.store_dropout_noise_ = False
        if self.store_dropout_noise_:
            self.dropout_noise_.AllocateGPUMemory(batch_size, num_pixels * self.num_channels_, self.name_ + " dropout")
        if self.is_output_:
            self.loss_ = LossFunction.ChooseLossFunction(self.loss_function_)
            self.performance_ = LossFunction.ChooseLossFunction(self.performance_metric_)
        if self.batch_normalize_:
            # src/layer.cc:264-278.  Not part of the flat parameter buffer: ConvNet::Save writes edges only (convnet.cc:669-680)
            C = self.num_channels_
            for m, what in ((self.gamma_, "gamma"), (self.beta_, "beta"), (self.grad_gamma_, "grad gamma"), (self.grad_beta_, "grad beta"),
                            (self.batch_mu_, "batch mu"), (self.batch_sigma_, "batch sigma"), (self.mu_, "mu"), (self.sigma_, "sigma")):
                m.AllocateGPUMemory(1, C, f"{self.name_} bn {what}")
            self.gamma_optimizer_.AllocateMemory(1, C)
            self.beta_optimizer_.AllocateMemory(1, C)
            self.gamma_.Set(1)
            self.beta_.Set(0)
            self.mu_.Set(0)
            self.sigma_.Set(1)
            for m in (self.grad_gamma_, self.grad_beta_, self.batch_mu_, self.batch_sigma_):
                m.Set(0)
        self.SetupSlices()

    # ---- batch normalisation: src/layer.cc:452-510 --------------------------------------------------------------------
    def ApplyBatchNormalization(self, train, relu=False):
        """Unfused: the reference's call sequence.  Fused (``self.fused``): bn_fprop_act, which also applies this layer's ReLU when
        ``relu`` (the caller then skips ApplyActivation)."""
        if self.fused:
            Matrix.BNFpropAct(self.state_, self.gamma_, self.beta_, self.mu_, self.sigma_, self.batch_mu_, self.batch_sigma_,
                              self.bn_f_, self.bn_epsilon_, train, relu)
            return
        assert not relu
        st = self.state_
        batch_size = st.GetRows()
        st.Reshape(-1, self.num_channels_)
        n = st.GetRows()
        inv_n = float(np.float32(1) / np.float32(n))   # 1.0f / n
        if train:
            st.SumRows(self.batch_mu_, 0, inv_n)
            st.AddRowVec(self.batch_mu_, -1)
            st.SqSumAxis(self.batch_sigma_, 0, inv_n, 0)
            self.batch_sigma_.Add(self.bn_epsilon_)
            self.batch_sigma_.Sqrt()
            st.DivideByRowVec(self.batch_sigma_)
            one_minus_f = float(np.float32(1) - np.float32(self.bn_f_))
            self.mu_.Mult(self.bn_f_)
            self.mu_.Add(self.batch_mu_, one_minus_f)
            self.sigma_.Mult(self.bn_f_)
            self.sigma_.Add(self.batch_sigma_, one_minus_f)
        else:
            st.AddRowVec(self.mu_, -1)
            st.DivideByRowVec(self.sigma_)
        st.MultByRowVec(self.gamma_)
        st.AddRowVec(self.beta_, 1)
        st.Reshape(batch_size, -1)

    def ApplyDerivativeofBatchNormalization(self, fused_steps=None):
        """The derivative and, as in the reference, the gamma / beta optimizer steps.  Fused: bn_bprop_fused (the state is only read);
        with ``fused_steps`` (a list) the plain steps are appended to it as data for the host's multi launch (optimizer.RunFusedSteps)
        instead of running here — nothing reads gamma or beta between here and the end of the step."""
        if self.fused:
            Matrix.BNBpropFused(self.deriv_, self.state_, self.gamma_, self.beta_, self.batch_sigma_, self.grad_gamma_, self.grad_beta_)
            for opt, g, p in ((self.gamma_optimizer_, self.grad_gamma_, self.gamma_), (self.beta_optimizer_, self.grad_beta_, self.beta_)):
                item = opt.PlanFusedStep(g, p) if fused_steps is not None else None
                if item is None:
                    opt.Optimize(g, p)
                else:
                    fused_steps.append(item)
            return
        st, dv = self.state_, self.deriv_
        batch_size = st.GetRows()
        dv.Reshape(-1, self.num_channels_)
        st.Reshape(-1, self.num_channels_)
        n = st.GetRows()
        st.AddRowVec(self.beta_, -1)
        st.DivideByRowVec(self.gamma_)
        dv.SumRows(self.grad_beta_, 0, float(np.float32(1) / np.float32(n)))
        Matrix.BNBpropInplace(dv, st, self.grad_gamma_)
        dv.MultByRowVec(self.gamma_)
        dv.DivideByRowVec(self.batch_sigma_)
        st.MultByRowVec(self.gamma_)
        st.AddRowVec(self.beta_, 1)
        st.Reshape(batch_size, -1)
        dv.Reshape(batch_size, -1)
        self.gamma_optimizer_.Optimize(self.grad_gamma_, self.gamma_)
        self.beta_optimizer_.Optimize(self.grad_beta_, self.beta_)

    # ---- activation / dropout ----------------------------------------------------------------------------
    def ApplyActivation(self):
        raise NotImplementedError

    def ApplyDerivativeOfActivation(self):
        raise NotImplementedError

    def ApplyDropout(self, train):
        if train:
            self.ApplyDropoutAtTrainTime()
        else:
            self.ApplyDropoutAtTestTime()

    def TrainDropoutScale(self):
        """What the units kept at train time are scaled by: 1 / (1 - p) with binary dropout and scale-up at train time, else 1 (Gaussian
        noise has mean 1)."""
        binary = self.dropprob_ > 0 and not self.gaussian_dropout_
        return 1.0 / (1 - self.dropprob_) if (binary and self.dropout_scale_up_at_train_time_) else 1.0

    def FusedGaussianDropout(self):
        """Whether this layer's Gaussian dropout runs through the fused pair of entries (the fused host's choice for every Gaussian
        layer: measured faster than the sequences it replaces at both shapes of profiles/gaussian_dropout_bench.json) —
        the one place that decides it."""
        return self.fused and self.gaussian_dropout_

    def ApplyGaussianDropout(self, act):
        """Fused host: Gaussian dropout in one pass, with the activation ``act`` (0 when something before has applied it, else
        ``gaussian_act``) in front; the call id stays with the layer for ApplyDerivativeofGaussianDropout."""
        self.gaussian_call_id_ = self.state_.GaussianDropout(self.dropprob_, self.max_act_gaussian_dropout_, act)

    def ApplyDerivativeofGaussianDropout(self, restore_state):
        """Fused host, hidden layers: dropout' and the activation's derivative at state / noise in one pass, the noise drawn again from the
        forward pass's call id.  Without ``restore_state`` the state is only read, so a weight gradient reading it on another stream
        needs no ordering; with it the state is left as the reference leaves it, state / noise, for whoever reads it afterwards
        (ConvNet.gaussian_restore_)."""
        self.deriv_.GaussianDropoutUndo(self.gaussian_call_id_, self.dropprob_, self.state_, self.gaussian_act, restore_state)

    def ApplyDropoutAtTrainTime(self):
        # src/layer.cc:367-397
        if self.dropprob_ > 0:
            if self.gaussian_dropout_:
                if self.FusedGaussianDropout():
                    self.ApplyGaussianDropout(0)
                    return
                self.dropout_noise_.FillWithRandn()
                self.dropout_noise_.Mult(self.dropprob_)
                self.dropout_noise_.Add(1)
                self.state_.Mult(self.dropout_noise_)
                if self.max_act_gaussian_dropout_ > 0:
                    self.state_.UpperBoundMod(self.max_act_gaussian_dropout_)   # |state| <= max_act
                return
            scale = self.TrainDropoutScale()
            if self.store_dropout_noise_:
                self.dropout_noise_.SampleBernoulli(1 - self.dropprob_)
                self.dropout_noise_.Mult(scale)
                self.state_.Mult(self.dropout_noise_)
            else:
                self.state_.Dropout(self.dropprob_, 0, scale)

    def ApplyDerivativeofDropout(self):
        # src/layer.cc:399-413
        if self.dropprob_ > 0:
            if self.gaussian_dropout_:
                # unfused (the fused host calls ApplyDerivativeofGaussianDropout instead).  An input layer takes no derivative
                if not self.is_input_:
                    self.deriv_.Mult(self.dropout_noise_)
                    self.state_.Divide(self.dropout_noise_)   # the activation's derivative is taken at the state before the noise
            elif self.store_dropout_noise_:
                self.deriv_.Mult(self.dropout_noise_)
            elif self.dropout_scale_up_at_train_time_:
                self.deriv_.Mult(self.TrainDropoutScale())

    def ApplyDropoutAtTestTime(self):
        if self.dropprob_ > 0 and not self.dropout_scale_up_at_train_time_:
            self.state_.Mult(1 - self.dropprob_)

    # ---- loss ---------------------------------------------------------------------------------------
    def GetPerformanceMetric(self):
        return self.performance_.GetLoss(self.state_, self.data_)

    def ComputeDeriv(self):
        self.loss_.GetLossDerivative(self.state_, self.data_, self.deriv_)
        if self.loss_function_weight_ != 1.0:
            self.deriv_.Mult(self.loss_function_weight_)

    def GetLoss(self):
        return self.loss_function_weight_ * self.loss_.GetLoss(self.state_, self.data_)


class LinearLayer(Layer):
    is_relu = False
    gaussian_act = 0   # the activation's code in gaussian_dropout / gaussian_dropout_undo (include/convnet_hip.h)

    def ApplyActivation(self):
        pass  # linear: nothing to do (src/layer.cc:530-532)

    def ApplyDerivativeOfActivation(self):
        pass

    def AllocateMemory(self, batch_size):
        super().AllocateMemory(batch_size)
        num_pixels = self.image_size_y_ * self.image_size_x_ * self.image_size_t_
        if self.is_output_:
            self.data_.AllocateGPUMemory(batch_size, num_pixels * self.num_channels_, self.name_ + " data")


class ReLULayer(LinearLayer):
    is_relu = True
    gaussian_act = 1

    def __init__(self, config):
        super().__init__(config)
        self.store_dropout_noise_ = False  # src/layer.cc:544-547: ReLU' zeroes dropped units

    def ApplyActivation(self):
        self.state_.LowerBound(0)

    def ApplyDerivativeOfActivation(self):
        self.deriv_.ApplyDerivativeOfReLU(self.state_)


class SoftmaxLayer(Layer):
    is_relu = False

    def AllocateMemory(self, batch_size):
        super().AllocateMemory(batch_size)
        if self.is_output_:
            self.data_.AllocateGPUMemory(batch_size, 1, self.name_ + " data")
        Matrix.RegisterTempMemory(batch_size)

    def ApplyActivation(self):
        self.state_.ApplySoftmax()

    def ApplyDerivativeOfActivation(self):
        raise SystemExit("Back prop through softmax is not implemented.")


class SoftmaxDistLayer(SoftmaxLayer):
    """Softmax against a target DISTRIBUTION per case (src/layer.cc:579-584)."""

    def AllocateMemory(self, batch_size):
        Layer.AllocateMemory(self, batch_size)
        numdims = self.state_.GetCols()
        Matrix.RegisterTempMemory(batch_size * numdims)   # for computing CE
        if self.is_output_:
            self.data_.AllocateGPUMemory(batch_size, numdims, self.name_ + " data")


class LogisticLayer(Layer):
    """src/layer.cc:586-602.  The dropout mask is not stored: ApplyDerivativeofDropout scales the derivative by 1 / (1 - p) and the
    logistic derivative y (1 - y) is then taken at the dropout-SCALED state, exactly 0 for a dropped unit — the reference's quirk, kept.
    (Gaussian dropout stores or redraws its noise like every other class: Layer.AllocateMemory.)"""
    is_relu = False
    gaussian_act = 2

    def __init__(self, config):
        super().__init__(config)
        self.store_dropout_noise_ = False

    def AllocateMemory(self, batch_size):
        super().AllocateMemory(batch_size)
        Matrix.RegisterTempMemory(batch_size)
        if self.is_output_:
            self.data_.AllocateGPUMemory(batch_size, self.num_channels_, self.name_ + " data")

    def ApplyActivation(self):
        self.state_.ApplyLogistic()

    def ApplyDerivativeOfActivation(self):
        self.deriv_.ApplyDerivativeOfLogistic(self.state_)
