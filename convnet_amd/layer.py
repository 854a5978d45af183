"""Layers — mirror of src/layer.{h,cc} for the hot path: Linear / ReLU / Logistic / Softmax / Softmax-distribution layers with
binary dropout, batch normalisation, their losses and metrics.  Slices, Gaussian dropout and the model-parallel state copies are
out of scope."""
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
        self.add_or_overwrite_state_ = True
        self.add_or_overwrite_deriv_ = True
        if config.layer_slice or self.gaussian_dropout_:
            raise SystemExit("layer_slice / gaussian_dropout are out of hot-path scope")
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

    def GetNumChannels(self, slice_=""):
        return self.num_channels_

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
        return self.state_

    def GetDeriv(self, slice_=""):
        return self.deriv_

    def GetData(self):
        return self.data_

    # add-or-overwrite bookkeeping: src/layer.cc:307-332
    def AddOrOverwriteState(self, slice_=""):
        v = self.add_or_overwrite_state_
        self.add_or_overwrite_state_ = False
        return v

    def AddOrOverwriteDeriv(self, slice_=""):
        v = self.add_or_overwrite_deriv_
        self.add_or_overwrite_deriv_ = False
        return v

    def ResetAddOrOverwrite(self):
        self.add_or_overwrite_state_ = True
        self.add_or_overwrite_deriv_ = True

    def UseBatchNormalization(self):
        return self.batch_normalize_

    def NotifyStart(self):
        # src/layer.cc:520-525
        if self.batch_normalize_:
            self.gamma_optimizer_.NotifyStart(self.gamma_)
            self.beta_optimizer_.NotifyStart(self.beta_)

    # ---- memory: src/layer.cc:252-288 ----------------------------------------------------------------
    def AllocateMemory(self, batch_size):
        num_pixels = self.image_size_y_ * self.image_size_x_ * self.image_size_t_
        self.state_.AllocateGPUMemory(batch_size, num_pixels * self.num_channels_, self.name_ + " state")
        self.deriv_.AllocateGPUMemory(batch_size, num_pixels * self.num_channels_, self.name_ + " deriv")
        for m in (self.state_, self.deriv_):
            m.SetShape4D(batch_size, self.image_size_x_, self.image_size_y_, self.num_channels_ * self.image_size_t_)
        if self.is_input_:
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
        """What the units kept at train time are scaled by: 1 / (1 - p) with dropout and scale-up at train time, else 1."""
        return 1.0 / (1 - self.dropprob_) if (self.dropprob_ > 0 and self.dropout_scale_up_at_train_time_) else 1.0

    def ApplyDropoutAtTrainTime(self):
        # src/layer.cc:367-397
        if self.dropprob_ > 0:
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
            if self.store_dropout_noise_:
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
    logistic derivative y (1 - y) is then taken at the dropout-SCALED state, exactly 0 for a dropped unit — the reference's quirk, kept."""
    is_relu = False

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
