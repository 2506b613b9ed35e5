/* Stand-in for libkev's DestroyDetector.h (the libkev submodule of the
 * reference is empty).  TEST INFRASTRUCTURE ONLY, written from scratch.
 *
 * What WSHandler::handleFrame needs: DESTROY_DETECTOR_SETUP() before the frame
 * callback, DESTROY_DETECTOR_CHECK(ret) after it.  If the callback deleted the
 * handler, the check returns `ret` without touching the dead object; otherwise
 * it restores the detector to the state it had before the setup, so that the
 * pair nests.
 *
 * Each setup places a watch on the caller's stack and pushes it on the
 * object's list; the destructor marks every watch on the list. */
#pragma once

namespace kev {

class DestroyDetector
{
public:
    struct Watch {
        bool destroyed = false;
        Watch* outer = nullptr;
    };

    DestroyDetector() = default;
    DestroyDetector(const DestroyDetector&) {}
    DestroyDetector& operator=(const DestroyDetector&) { return *this; }

    ~DestroyDetector()
    {
        for (Watch* w = watch_; w; w = w->outer) w->destroyed = true;
    }

    void pushWatch(Watch& w) { w.outer = watch_; watch_ = &w; }
    void popWatch(Watch& w) { watch_ = w.outer; }

private:
    Watch* watch_ = nullptr;
};

} // namespace kev

#define DESTROY_DETECTOR_SETUP() \
    kev::DestroyDetector::Watch __dd_watch; \
    this->pushWatch(__dd_watch)

#define DESTROY_DETECTOR_CHECK(ret) \
    if (__dd_watch.destroyed) return ret; \
    this->popWatch(__dd_watch)

#define DESTROY_DETECTOR_CHECK_VOID() \
    if (__dd_watch.destroyed) return; \
    this->popWatch(__dd_watch)
