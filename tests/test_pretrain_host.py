"""not gpu: the best-epoch rule of pretrain_clf (src/pretrain_clf.py:126-129) on hand-written epoch sequences.  The expected dicts are
worked out by hand from the rule: record the epoch when its validation metric is greater than the recorded one, or equal with a smaller
validation loss; the dict starts at 0 everywhere (src/utils/utils.py:13-14)."""
from dp_gsat_amd.pretrain import METRIC_KEYS, init_clf_metric_dict, update_best_clf


def _dict(epoch, valid_loss, train, valid, test):
    return dict(zip(METRIC_KEYS, (epoch, valid_loss, train, valid, test)))


def _run(epochs):
    d = init_clf_metric_dict()
    recorded = [update_best_clf(d, e, *row) for e, row in enumerate(epochs)]
    return d, recorded


def test_initial_dict_has_the_references_keys():
    assert init_clf_metric_dict() == {"metric/best_clf_epoch": 0, "metric/best_clf_valid_loss": 0, "metric/best_clf_train": 0,
                                      "metric/best_clf_valid": 0, "metric/best_clf_test": 0}


def test_first_epoch_is_recorded_when_its_metric_is_positive():
    # rows: (train, valid, test, valid_loss).  0.5 > 0: recorded
    d, rec = _run([(0.6, 0.5, 0.4, 0.9)])
    assert rec == [True] and d == _dict(0, 0.9, 0.6, 0.5, 0.4)


def test_first_epoch_with_metric_zero_is_not_recorded():
    # 0 > 0 is false; 0 == 0 and 0.7 < 0 is false: the dict stays as it started
    d, rec = _run([(0.3, 0.0, 0.2, 0.7)])
    assert rec == [False] and d == init_clf_metric_dict()


def test_strict_improvement_wins_whatever_the_loss():
    # epoch 1: 0.75 > 0.5 with a LARGER loss: recorded.  epoch 2: 0.7 < 0.75: not
    d, rec = _run([(0.6, 0.5, 0.4, 0.9), (0.7, 0.75, 0.65, 1.5), (0.9, 0.7, 0.8, 0.1)])
    assert rec == [True, True, False] and d == _dict(1, 1.5, 0.7, 0.75, 0.65)


def test_tie_is_won_on_a_smaller_loss_and_lost_otherwise():
    # epoch 1: 0.5 == 0.5 and 0.8 < 0.9: recorded.  epoch 2: 0.5 == 0.5 and 0.8 < 0.8 false: not.  epoch 3: the same with 0.85: not
    d, rec = _run([(0.6, 0.5, 0.4, 0.9), (0.61, 0.5, 0.45, 0.8), (0.62, 0.5, 0.99, 0.8), (0.63, 0.5, 0.99, 0.85)])
    assert rec == [True, True, False, False] and d == _dict(1, 0.8, 0.61, 0.5, 0.45)


def test_nan_metric_is_never_recorded():
    # NaN compares false both ways (an epoch whose ROC-AUC has no scorable task)
    d, rec = _run([(0.6, float("nan"), 0.4, 0.9), (0.6, 0.5, 0.4, 0.9)])
    assert rec == [False, True] and d == _dict(1, 0.9, 0.6, 0.5, 0.4)
