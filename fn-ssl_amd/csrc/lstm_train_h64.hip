// The LSTM training kernels (forward with reserve, BPTT; lstm_train.h) for hidden size 64: the full-band and offline
// narrow-band layers of IPDnet at hidden_size 128, the reference's default.  A translation unit of its own, like
// lstm_train_h256.hip, so that the hidden sizes compile in parallel.
#include "lstm_train.h"

namespace fnssl_lstm {
template int launch_bwd<64>(int, int, const BwdParams&, int, const LaunchCtx&);
template int launch_save<64>(int, int, const LstmParams&, int, int, const LaunchCtx&);
}  // namespace fnssl_lstm
