"""Loss functions — mirror of src/loss_functions.{h,cc} for the hot path's output layers: squared and linear error, the softmax, softmax-distribution
and logistic cross entropies and the two classification metrics."""
from .matrix import Matrix


class LossFunction:
    @staticmethod
    def ChooseLossFunction(lf):
        # src/loss_functions.cc:5-36
        table = {"SQUARED_ERROR": SquaredError, "LINEAR_ERROR": LinearError, "CROSS_ENTROPY_MULTINOMIAL": CrossEntropyMultinomial,
                 "CROSS_ENTROPY_MULTINOMIAL_DISTRIBUTED": CrossEntropyDistributed, "CROSS_ENTROPY_BINARY": CrossEntropyBinary,
                 "CLASSIFICATION_MULTINOMIAL": ClassificationMultinomial, "CLASSIFICATION_BINARY": ClassificationBinary}
        if lf not in table:
            raise SystemExit(f"Unknown loss function {lf}")
        return table[lf]()


class SquaredError(LossFunction):
    def GetLoss(self, y, t):
        temp = Matrix()
        Matrix.GetTemp(t.GetRows(), t.GetCols(), temp)
        y.Subtract(t, temp)
        norm = temp.EuclidNorm()
        return 0.5 * norm * norm

    def GetLossDerivative(self, y, t, dLbydy):
        y.Subtract(t, dLbydy)


class LinearError(LossFunction):
    def GetLoss(self, y, t):
        temp = Matrix()
        Matrix.GetTemp(t.GetRows(), t.GetCols(), temp)
        y.Subtract(t, temp)
        return temp.Sum()

    def GetLossDerivative(self, y, t, dLbydy):
        dLbydy.Set(1)


class CrossEntropyMultinomial(LossFunction):
    def GetLoss(self, y, t):
        temp = Matrix()
        Matrix.GetTemp(t.GetRows(), 1, temp)
        Matrix.SoftmaxCE(y, t, temp)
        return temp.Sum()

    def GetLossDerivative(self, y, t, dLbydy):
        Matrix.SoftmaxCEDeriv(y, t, dLbydy)


class CrossEntropyBinary(LossFunction):
    def GetLoss(self, y, t):
        return 0.0   # "Not implemented" in the reference (src/loss_functions.cc:88-91): it reports 0, and so does this host

    def GetLossDerivative(self, y, t, dLbydy):
        Matrix.LogisticCEDeriv(y, t, dLbydy)


class CrossEntropyDistributed(LossFunction):
    def GetLoss(self, y, t):
        temp = Matrix()
        Matrix.GetTemp(t.GetRows(), t.GetCols(), temp)
        Matrix.SoftmaxDistCE(y, t, temp)
        return temp.Sum()

    def GetLossDerivative(self, y, t, dLbydy):
        y.Subtract(t, dLbydy)


class ClassificationMultinomial(LossFunction):
    def GetLoss(self, y, t):
        temp = Matrix()
        Matrix.GetTemp(t.GetRows(), 1, temp)
        Matrix.SoftmaxCorrect(y, t, temp)
        return temp.Sum()

    def GetLossDerivative(self, y, t, dLbydy):
        dLbydy.Set(0)


class ClassificationBinary(LossFunction):
    def GetLoss(self, y, t):
        temp = Matrix()
        Matrix.GetTemp(t.GetRows(), 1, temp)
        Matrix.LogisticCorrect(y, t, temp)
        return temp.Sum()

    def GetLossDerivative(self, y, t, dLbydy):
        dLbydy.Set(0)
